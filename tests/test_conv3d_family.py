"""CPU (host emulator): every tuned 3-D MFMA convolution kernel (csrc/conv_kernels.hip, csrc/conv_bf16x3_kernels.hip), entry point by entry
point, against the float64 restatement of tests/conv3d_ref.py.  tests/test_conv3d_family_gpu.py runs the same case functions on the device.

1. Every row of MVS_CONV_TABLE (12) and MVS_DECONV_TABLE (6) in the formats fp32, bf16x3, split, f16x2 and f16 through ops.conv3d_bn_relu /
   ops.deconv3d_bn_relu_add, batch 2, at one input voxel, a shape below one tile on every axis, an exact multiple of the tile (two z-tiles)
   and a ragged shape with two tiles per axis (odd H and W on the strided rows); the tile sizes come from csrc/conv_cfg.h.  The two kd = 1
   rows take D = 1 there and one more ragged shape with D = 3 (three z-tiles).  relu = False once per conv row, ops.deconv3d_linear once
   per transposed row (both bf16x3), the transposed rows with and without skip.
   REFUSED lists the (row, format) pairs the dispatch refuses: NONE - every row has a kernel in every format (the literal set is empty and
   a pair that starts to refuse fails here, as does one listed that runs).
2. ops.deconv3d_prob (both depth strides; bf16x3, split, f16x2, f16) and ops.conv3d_logits (bf16x3, split, f16x2; f16 / f16mix give the
   f16x2 bits) at the ragged shape against the restated heads.
3. The persistent kernels over several tiles per block: the emulator reports three resident blocks, so 4 / 7 / 10 tiles give runs of
   2 + 2 + (a block that returns), 3 + 3 + 1 and 4 + 4 + 2.  On the device the same case runs with more than 8 x CU count tiles.

Bars (none comes from the kernels' output):
  split-bf16 formats   max |got - ref| <= LAYER_BAR x max(1, max |ref|), LAYER_BAR = 3e-5 (tests/test_fpn.py, test_fmt.py, test_vit.py).  Its
                       condition - the float64 reference on x and w each rounded to hi + lo bf16 stays below HALF the bar from the plain
                       one - is asserted from the restatement alone in test_format_alone_leaves_half_the_bar.
  fp32                 per element |got - ref| <= K 2^-24 S: S = sum |x| |w| of that element, K = products per output (taps x Cin; the
                       transposed rows: the largest parity class's taps x Cin) - the first-order worst case of an fp32 accumulation chain.
  fp16 formats         the reference sees the format's operand model (conv3d_ref).  (a) per element |got - ref| <= 2^-11 |ref| + K 2^-24 S
                       (half an fp16 ulp of the stored value + the chain); (b) at most 2 % of the fp16 bits differ from fp16(ref) (the cap of
                       test_feature_heads for "the reference rounded once").  (b) is a share: it is taken over each (row, format)'s pooled
                       elements and over every single tensor of at least 2048 elements - on the 32 outputs of the one-voxel shape one
                       differing element is already 3 %, which says nothing about a share.
  fused-head logits    fp32 in every format.  split-bf16 formats: LAYER_BAR.  fp16 formats: |got - ref| <= 2^-11 A + K 2^-24 S' with
                       A = sum_c |y_c prob_w_c| and S' = sum_c |prob_w_c| (S_c + |bias_c| + |skip_c|) + |prob_b|.  Derivation: the layer's
                       output y_c carries at most the fp16 formats' own per-element error 2^-11 |y_c| + K 2^-24 S_c (the kernel keeps y_c
                       in fp32, so the first term is slack it does not use); the head multiplies that by |prob_w_c| and sums it, which gives
                       2^-11 A + K 2^-24 sum_c |prob_w_c| S_c; the head's own 8 products, the bias, skip and prob_b adds are 11 more
                       roundings of partial sums bounded by S', far fewer than K >= 128.  ops.conv3d_logits has no stored y: its bar is the
                       chain term K 2^-24 S alone.

Inputs: randn activations, weights randn / sqrt(taps x Cin), randn bias and skip: outputs are O(5), far from the fp16 clamp.

Worst figures of the emulator run (pytest -s prints each):
  split-bf16 (x max(1, max|ref|), bar 3e-5)   bf16x3 8.5e-6, split 9.1e-6; deconv3d_prob 2.0e-6 / 3.5e-6, conv3d_logits 4.3e-6 / 4.3e-6;
                                               the two-term operands alone 6.2e-6 (half the bar: 1.5e-5)
  fp32 (fraction of K 2^-24 S, bar 1)          0.11 (16 -> 8 transposed, depth stride 2: a one-tap parity class has 16 products, K = 128)
  fp16 (a) (fraction of its bar, bar 1)        f16x2 0.99, f16 0.99 (an element rounded at the very half ulp sits at 1 minus the chain's
                                               share, by construction); deconv3d_prob 7.3e-4, conv3d_logits 1.4e-2
  fp16 (b) (share of differing bits, cap 2 %)  f16x2 0.17 %, f16 0.12 % pooled per row, 0.18 % / 0.12 % on a single tensor; the small
                                               tensors of part 3: 0.35 % pooled
"""
import pytest
import torch

import conv3d_ref as R
from conv3d_ref import F16_FORMATS, FORMATS, LAYER_BAR, SPLIT_BF16_FORMATS
from mvsformerplusplus_amd import ops, packing
from mvsformerplusplus_amd._lib import MvsHipError

# (Cin, Cout, kd, stride) and (Cin, Cout, sd): the literal tables this file was written for
CONV_ROWS = [(16, 16, 3, (1, 1, 1)), (32, 32, 3, (1, 1, 1)), (64, 64, 3, (1, 1, 1)), (8, 16, 3, (1, 1, 1)), (8, 16, 3, (2, 2, 2)), (16, 32, 3, (2, 2, 2)),
             (32, 64, 3, (2, 2, 2)), (8, 16, 3, (1, 2, 2)), (16, 32, 3, (1, 2, 2)), (32, 64, 3, (1, 2, 2)), (16, 16, 1, (1, 1, 1)), (16, 8, 1, (1, 1, 1))]
DECONV_ROWS = [(64, 32, 2), (32, 16, 2), (16, 8, 2), (64, 32, 1), (32, 16, 1), (16, 8, 1)]
REFUSED = set()                                            # (kind, row, format) the dispatch refuses: none
MFMA = ("bf16x3", "split", "f16x2", "f16")
# the instantiations that run the persistent tile loop, and in which formats
PERSISTENT_CONV = {(8, 16, 3, (2, 2, 2)): MFMA, (8, 16, 3, (1, 2, 2)): MFMA, (8, 16, 3, (1, 1, 1)): MFMA,
                   (16, 16, 3, (1, 1, 1)): ("f16",), (16, 16, 1, (1, 1, 1)): ("f16",), (16, 8, 1, (1, 1, 1)): ("f16",)}
PERSISTENT_DECONV = {(16, 8, 2): MFMA, (16, 8, 1): MFMA}
EMULATOR_BLOCKS = 3
BITS_MIN_ELEMS = 2048


def conv_cfg(key):
    return next(r for r in R.tile_tables()[0] if (r[0], r[1], r[2], r[3:6]) == key)


def deconv_cfg(key):
    return next(r for r in R.tile_tables()[1] if r[:3] == key)


# ---------------------------------------------------------------------------------------------------------------- running one layer
class Figures:
    """Worst figure per (format, kind of figure) and the pooled fp16 bit counts of one test."""

    def __init__(self):
        self.worst, self.bits = {}, {}

    def note(self, fmt, name, value):
        self.worst[(fmt, name)] = max(self.worst.get((fmt, name), 0.0), value)

    def show(self, title):
        print("%s: %s" % (title, ", ".join("%s %s %.3g" % (f, n, v) for (f, n), v in sorted(self.worst.items()))))

    def close_bits(self):
        for fmt, (bad, n) in self.bits.items():
            self.note(fmt, "bits", bad / n)
            assert bad <= R.F16_BITS_CAP * n, (fmt, "fp16 bits differing from the once-rounded reference", bad, n)


def judge(figs, fmt, got, ref, S, K, what):
    """One stored layer output against its bar (module docstring)."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), what
    if fmt in SPLIT_BF16_FORMATS:
        fig = R.split_figure(got, ref)
        figs.note(fmt, "layer", fig)
        assert fig <= LAYER_BAR, (what, fmt, fig)
    elif fmt == "fp32":
        fig = R.chain_figure(got, ref, S, K)
        figs.note(fmt, "chain", fig)
        assert fig <= 1.0, (what, fmt, fig)
    else:
        assert got.dtype == torch.float16, (what, got.dtype)
        fig = R.chain_figure(got, ref, S, K, rel=2.0 ** -11 * ref.abs())
        figs.note(fmt, "chain", fig)
        assert fig <= 1.0, (what, fmt, fig)
        share = R.f16_bits_share(got, ref)
        bad, n = figs.bits.get(fmt, (0, 0))
        figs.bits[fmt] = (bad + round(share * got.numel()), n + got.numel())
        if got.numel() >= BITS_MIN_ELEMS:
            figs.note(fmt, "bits/tensor", share)
            assert share <= R.F16_BITS_CAP, (what, fmt, share)


def judge_logits(figs, fmt, got, ref, S1, K, what, A=None):
    """Fused-head logits (fp32 in every format) against their bar."""
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (what, tuple(got.shape), got.dtype)
    if fmt in SPLIT_BF16_FORMATS:
        fig = R.split_figure(got, ref)
        assert fig <= LAYER_BAR, (what, fmt, fig)
    else:
        fig = R.chain_figure(got, ref, S1, K, rel=None if A is None else 2.0 ** -11 * A)
        assert fig <= 1.0, (what, fmt, fig)
    figs.note(fmt, "head", fig)


def feed(fmt, t, device):
    """A channel-last fp32 tensor in the activation form of `fmt`, on the device."""
    if t is None:
        return None
    t = t.half() if fmt in F16_FORMATS else ops.to_split(t) if fmt == "split" else t
    return t.to(device)


def read(fmt, t):
    t = t.cpu()
    return ops.from_split(t) if fmt == "split" else t


def pack_conv(fmt, w, ch, device):
    if fmt == "fp32":
        return packing.pack_conv_weights(w, ch).to(device)
    return (packing.f16x2(packing.pack_conv_weights_bf16x3, w, ch) if fmt in F16_FORMATS else packing.pack_conv_weights_bf16x3(w, ch)).to(device)


def pack_deconv(fmt, w, sd, device):
    if fmt == "fp32":
        return packing.pack_deconv_weights(w).to(device)
    return (packing.f16x2(packing.pack_deconv_weights_bf16x3, w, sd) if fmt in F16_FORMATS else packing.pack_deconv_weights_bf16x3(w, sd)).to(device)


def conv_inputs(cfg, B, shape, seed):
    cin, cout, kd = cfg[:3]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, *shape, cin, generator=g)
    w = torch.randn(cout, cin, kd, 3, 3, generator=g) / (kd * 9 * cin) ** 0.5
    return x, w, packing.pad_bias(torch.randn(cout, generator=g))


def deconv_inputs(cfg, B, shape, seed):
    cin, cout, sd = cfg[:3]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, *shape, cin, generator=g)
    w = torch.randn(cin, cout, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    skip = torch.randn(B, shape[0] * sd, 2 * shape[1], 2 * shape[2], cout, generator=g)
    return x, w, packing.pad_bias(torch.randn(cout, generator=g)), skip


def run_conv(fmt, cfg, x, w, bias, device, relu=True):
    cin, cout, kd, sd, sh, sw, TD, TH, ch = cfg
    y = ops.conv3d_bn_relu(feed(fmt, x, device), pack_conv(fmt, w, ch, device), bias.to(device), cout, kd, (sd, sh, sw), relu, R.CODE[fmt])
    return read(fmt, y)


def run_deconv(fmt, cfg, x, w, bias, skip, device):
    cin, cout, sd = cfg[:3]
    y = ops.deconv3d_bn_relu_add(feed(fmt, x, device), pack_deconv(fmt, w, sd, device), bias.to(device), cout, sd, feed(fmt, skip, device), R.CODE[fmt])
    return read(fmt, y)


def refs(fn, fmts):
    """{format: fn(format)} computed once per operand model."""
    made, out = {}, {}
    for fmt in fmts:
        k = R.model_key(fmt)
        if k not in made:
            made[k] = fn(fmt)
        out[fmt] = made[k]
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. the whole table
def conv_shapes(cfg):
    """Input (D, H, W) of part 1 for one conv row (module docstring)."""
    cin, cout, kd, sd, sh, sw, TD, TH, ch = cfg
    inp = lambda o, s: (o - 1) * s + 1                    # the smallest input with o outputs: odd at stride 2, where (I - 1) / 2 + 1 != I / 2
    if kd == 1:                                           # the 2-D rows: D = 1, and one more shape with three z-tiles
        return [(1, 1, 1), (1, TH - 1, 5), (1, 2 * TH, 16), (1, TH + 1, 19), (3, TH + 1, 19)]
    return [(1, 1, 1), (inp(max(1, TD - 1), sd), inp(TH - 1, sh), inp(5, sw)), (2 * TD * sd, TH * sh, 16 * sw),
            (inp(TD + 1, sd), inp(TH + 1, sh), inp(19, sw))]


def deconv_shapes(cfg):
    cin, cout, sd, TDM, THM = cfg
    return [(1, 1, 1), (max(1, TDM - 1), max(1, THM - 1), 5), (2 * TDM, THM, 16), (TDM + 1, THM + 1, 19)]


def check_shapes(tiles_of, cfg, shapes, T):
    """The shapes are what part 1 asks for: below one tile, exact multiples with two z-tiles, ragged with two tiles per axis."""
    assert tiles_of(*shapes[1], cfg) == (1, 1, 1)
    assert tiles_of(*shapes[2], cfg)[0] == 2 or T[0] == 1
    assert all(n >= 2 for n in tiles_of(*shapes[-1], cfg))


def case_conv_row(device, key, formats=FORMATS):
    """One row of MVS_CONV_TABLE in every format at the seam shapes.  -> {format: "run" | "refused"}."""
    cfg = conv_cfg(key)
    cin, cout, kd, sd, sh, sw, TD, TH, ch = cfg
    K = R.conv_products(cfg)
    shapes = conv_shapes(cfg)
    check_shapes(R.conv_ntiles, cfg, shapes, (TD, TH))
    if sh == 2:
        assert shapes[-1][1] % 2 == 1 and shapes[-1][2] % 2 == 1 and shapes[2][2] % 32 == 0
    figs, state = Figures(), {}
    for si, shape in enumerate(shapes):
        x, w, bias = conv_inputs(cfg, 2, shape, 100 + si)
        ref = refs(lambda f: R.conv(R.model_x(f, x), R.model_w(f, w), bias, (sd, sh, sw)), formats)
        for fmt in formats:
            if ("conv", key, fmt) in REFUSED:
                with pytest.raises(MvsHipError):
                    run_conv(fmt, cfg, x, w, bias, device)
                state[fmt] = "refused"
                continue
            judge(figs, fmt, run_conv(fmt, cfg, x, w, bias, device), *ref[fmt], K, ("conv", key, shape))
            state[fmt] = "run"
        if si == len(shapes) - 1 and "bf16x3" in formats:
            yl, S = R.conv(x, w, bias, (sd, sh, sw), relu=False)
            got = run_conv("bf16x3", cfg, x, w, bias, device, relu=False)
            assert float(got.min()) < 0.0, "relu = False must leave negative outputs"
            judge(figs, "bf16x3", got, yl, S, K, ("conv, linear", key, shape))
    figs.close_bits()
    figs.show("conv %s" % (key,))
    return state, figs


def case_deconv_row(device, key, formats=FORMATS):
    """One row of MVS_DECONV_TABLE in every format at the seam shapes, with and without skip, and ops.deconv3d_linear once."""
    cfg = deconv_cfg(key)
    cin, cout, sd, TDM, THM = cfg
    K = R.deconv_products(cfg)
    shapes = deconv_shapes(cfg)
    check_shapes(R.deconv_ntiles, cfg, shapes, (TDM, THM))
    figs, state = Figures(), {}
    for si, shape in enumerate(shapes):
        x, w, bias, skip = deconv_inputs(cfg, 2, shape, 200 + si)
        for sk in (None, skip):
            ref = refs(lambda f: R.deconv(R.model_x(f, x), R.model_w(f, w), bias, sd, skip=None if sk is None else R.model_x(f, sk)), formats)
            for fmt in formats:
                if ("deconv", key, fmt) in REFUSED:
                    with pytest.raises(MvsHipError):
                        run_deconv(fmt, cfg, x, w, bias, sk, device)
                    state[fmt] = "refused"
                    continue
                judge(figs, fmt, run_deconv(fmt, cfg, x, w, bias, sk, device), *ref[fmt], K, ("deconv", key, shape, sk is not None))
                state[fmt] = "run"
        if si == len(shapes) - 1 and "bf16x3" in formats:
            zero = torch.zeros_like(bias)
            yl, S = R.deconv(x, w, zero, sd, relu=False)
            got = ops.deconv3d_linear(x.to(device), pack_deconv("bf16x3", w, sd, device), zero.to(device), cout, sd, R.CODE["bf16x3"]).cpu()
            assert float(got.min()) < 0.0, "deconv3d_linear must leave negative outputs"
            judge(figs, "bf16x3", got, yl, S, K, ("deconv3d_linear", key, shape))
    figs.close_bits()
    figs.show("deconv %s" % (key,))
    return state, figs


def test_tables_are_the_literal_lists(emu):
    """The rows this file runs are the rows the library has: csrc/conv_cfg.h, the dispatch's own answer (ops.*_is_tuned over a grid of
    candidate layers) and the literal lists agree, 12 + 6 rows.  A row added without a test fails here."""
    conv, deconv = R.tile_tables()
    assert [(r[0], r[1], r[2], r[3:6]) for r in conv] == CONV_ROWS and len(CONV_ROWS) == 12
    assert [r[:3] for r in deconv] == DECONV_ROWS and len(DECONV_ROWS) == 6
    chans, strides = (4, 8, 16, 24, 32, 64, 128), [(a, b, c) for a in (1, 2) for b in (1, 2) for c in (1, 2)]
    tuned = {(ci, co, kd, s) for ci in chans for co in chans for kd in (1, 3, 5) for s in strides if ops.conv3d_is_tuned(ci, co, kd, s)}
    assert tuned == set(CONV_ROWS)
    assert {(ci, co, sd) for ci in chans for co in chans for sd in (1, 2, 3) if ops.deconv3d_is_tuned(ci, co, sd)} == set(DECONV_ROWS)
    assert all(k[1] in CONV_ROWS and k[2] in FORMATS for k in REFUSED if k[0] == "conv")
    assert all(k[1] in DECONV_ROWS and k[2] in FORMATS for k in REFUSED if k[0] == "deconv")


def test_persistent_lists_follow_the_kernel_rule():
    """PERSISTENT_CONV / PERSISTENT_DECONV against the rule of BfConv::PERSIST (Cin = 8 or one weight term, one channel pass, the weight
    fragments in at most 64 registers) and launch_deconv_bf (16 -> 8), evaluated on the table of csrc/conv_cfg.h."""
    conv, deconv = R.tile_tables()
    want = {}
    for cin, cout, kd, sd, sh, sw, TD, TH, ch in conv:
        nstep, mrep = R.ceil_div(kd * 9 * (ch // 8), 4), R.ceil_div(cout, 16)
        fmts = tuple(f for f in MFMA if (cin == 8 or f == "f16") and cin == ch and nstep * mrep * (4 if f == "f16" else 8) <= 64)
        if fmts:
            want[(cin, cout, kd, (sd, sh, sw))] = fmts
    assert want == PERSISTENT_CONV
    assert {r[:3]: MFMA for r in deconv if r[:2] == (16, 8)} == PERSISTENT_DECONV


@pytest.mark.parametrize("key", CONV_ROWS, ids=lambda k: "%dto%d_k%d_s%d%d%d" % (k[0], k[1], k[2], *k[3]))
def test_conv_row(emu, key):
    state, _ = case_conv_row(emu, key)
    assert set(state) == set(FORMATS) and all((v == "refused") == (("conv", key, f) in REFUSED) for f, v in state.items())


@pytest.mark.parametrize("key", DECONV_ROWS, ids=lambda k: "%dto%d_sd%d" % k)
def test_deconv_row(emu, key):
    state, _ = case_deconv_row(emu, key)
    assert set(state) == set(FORMATS) and all((v == "refused") == (("deconv", key, f) in REFUSED) for f, v in state.items())


def test_format_alone_leaves_half_the_bar():
    """The condition for LAYER_BAR: on the ragged shape of every row, the float64 reference with x and w each rounded to hi + lo bf16
    stays below half the bar from the plain float64 reference (from the restatement alone, no kernel runs)."""
    worst = 0.0
    for key in CONV_ROWS:
        cfg = conv_cfg(key)
        x, w, bias = conv_inputs(cfg, 2, conv_shapes(cfg)[-1], 100 + len(conv_shapes(cfg)) - 1)
        ref = R.conv(x, w, bias, key[3])[0]
        worst = max(worst, R.split_figure(R.conv(R.two_term_bf16(x), R.two_term_bf16(w), bias, key[3])[0], ref))
    for key in DECONV_ROWS:
        cfg = deconv_cfg(key)
        x, w, bias, skip = deconv_inputs(cfg, 2, deconv_shapes(cfg)[-1], 203)
        ref = R.deconv(x, w, bias, key[2], skip=skip)[0]
        worst = max(worst, R.split_figure(R.deconv(R.two_term_bf16(x), R.two_term_bf16(w), bias, key[2], skip=R.two_term_bf16(skip))[0], ref))
    print("two-term bf16 operands alone: %.3g x max(1, max|ref|) (half the bar: %g)" % (worst, LAYER_BAR / 2))
    assert worst <= LAYER_BAR / 2


# ---------------------------------------------------------------------------------------------------------------- 2. the fused heads
def run_prob(fmt, cfg, x, w, bias, skip, pw, pb, device):
    return ops.deconv3d_prob(feed(fmt, x, device), pack_deconv(fmt, w, cfg[2], device), bias.to(device), cfg[2], feed(fmt, skip, device),
                             pw.to(device), pb.to(device), R.CODE[fmt]).cpu()


def prob_reference(fmt, cfg, x, w, bias, skip, pw, pb):
    """-> (logits, S', A) of the fused head on the operand model of `fmt` (module docstring: fused-head logits)."""
    y, S = R.deconv(R.model_x(fmt, x), R.model_w(fmt, w), bias, cfg[2], skip=R.model_x(fmt, skip))
    logits, A = R.prob_head(y, pw, pb)
    S1 = ((S + bias[:8].double().abs() + R.model_x(fmt, skip).abs()) * pw.double().abs()).sum(-1) + float(pb.abs())
    return logits, S1, A


def case_deconv_prob(device, sd, shape=None, B=2, formats=MFMA, figs=None):
    """ops.deconv3d_prob: the persistent 16 -> 8 layer + skip + the 1x1x1 head in its epilogue."""
    cfg = deconv_cfg((16, 8, sd))
    shape = shape or deconv_shapes(cfg)[-1]
    figs = figs or Figures()
    x, w, bias, skip = deconv_inputs(cfg, B, shape, 300 + sd)
    g = torch.Generator().manual_seed(310 + sd)
    pw, pb = torch.randn(8, generator=g), torch.randn(1, generator=g)
    ref = refs(lambda f: prob_reference(f, cfg, x, w, bias, skip, pw, pb), formats)
    for fmt in formats:
        logits, S1, A = ref[fmt]
        judge_logits(figs, fmt, run_prob(fmt, cfg, x, w, bias, skip, pw, pb, device), logits, S1, R.deconv_products(cfg), ("deconv3d_prob", sd, fmt, shape),
                     A=A if fmt in F16_FORMATS else None)
    with pytest.raises(MvsHipError):                                          # the exact-fp32 layer has no fused head
        run_prob("fp32", cfg, x, w, bias, skip, pw, pb, device)
    figs.show("deconv3d_prob sd = %d %s" % (sd, shape))
    return figs


def case_conv_logits(device):
    """ops.conv3d_logits: the persistent 8 -> 16 stride-1 kernel with the planar store of row 0, weights as _RegNetBase.packed_all packs
    them (row 0 of 16 real, the rest zero)."""
    from mvsformerplusplus_amd import _lib
    cfg = conv_cfg((8, 16, 3, (1, 1, 1)))
    shape = conv_shapes(cfg)[-1]
    g = torch.Generator().manual_seed(320)
    x = torch.randn(2, *shape, 8, generator=g)
    w1 = torch.randn(8, 3, 3, 3, generator=g) / 216 ** 0.5
    w16 = torch.zeros(16, 8, 3, 3, 3)
    w16[0] = w1
    zero = torch.zeros(16)
    figs, got = Figures(), {}
    for fmt in ("bf16x3", "split", "f16x2"):
        ref, S = R.head3(R.model_x(fmt, x), R.model_w(fmt, w1))
        got[fmt] = ops.conv3d_logits(feed(fmt, x, device), pack_conv(fmt, w16, 8, device), zero.to(device), R.CODE[fmt]).cpu()
        judge_logits(figs, fmt, got[fmt], ref, S, 216, ("conv3d_logits", fmt))
    for code in (_lib.PREC_F16, _lib.PREC_F16MIX):                            # the entry point promotes them to both weight terms
        assert torch.equal(ops.conv3d_logits(feed("f16x2", x, device), pack_conv("f16x2", w16, 8, device), zero.to(device), code).cpu(), got["f16x2"])
    with pytest.raises(MvsHipError):
        ops.conv3d_logits(x.to(device), pack_conv("bf16x3", w16, 8, device), zero.to(device), _lib.PREC_FP32)
    figs.show("conv3d_logits %s" % (shape,))
    return figs


@pytest.mark.parametrize("sd", [2, 1])
def test_deconv_prob(emu, sd):
    case_deconv_prob(emu, sd)


def test_conv_logits(emu):
    case_conv_logits(emu)


# ---------------------------------------------------------------------------------------------------------------- 3. the persistent tile loop
def flat_id(v):
    """pytest id of a row key: the numbers of its (nested) tuple joined by underscores."""
    return v if isinstance(v, str) else "_".join(flat_id(i) for i in v) if isinstance(v, tuple) else str(v)


def persistent_instantiations():
    return [("conv", k) for k in PERSISTENT_CONV] + [("deconv", k) for k in PERSISTENT_DECONV]


def tiles_shape(kind, key, tiles):
    """The smallest input (D, H, W) with tiles = (tz, ty, tx) tiles per batch item: a ragged last tile on every axis with more than one."""
    if kind == "conv":
        cfg = conv_cfg(key)
        T, s = (cfg[6], cfg[7], 16), cfg[3:6]
        shape = tuple(((n - 1) * t + 1 - 1) * st + 1 for n, t, st in zip(tiles, T, s))
        assert R.conv_ntiles(*shape, cfg) == tuple(tiles), (key, shape, tiles)
    else:
        cfg = deconv_cfg(key)
        shape = tuple((n - 1) * t + 1 for n, t in zip(tiles, (cfg[3], cfg[4], 16)))
        assert R.deconv_ntiles(*shape, cfg) == tuple(tiles), (key, shape, tiles)
    return shape


def case_persistent(device, kind, key, tiles, B, resident, formats=None, run=None):
    """One persistent instantiation at `tiles` = (tz, ty, tx) tiles per batch item, more than the `resident` blocks the launch gets:
    every working block walks a run of at least two tiles (the prefetch of tile + 1, the second barrier per tile), the last run is
    ragged or a block returns without work.  The transposed rows run with skip, and the fused head once.  run(call) -> the output of
    call(); the device file passes one that repeats the call, on a second stream too, and asserts bit identity."""
    run = run or (lambda call: call())
    formats = formats or (PERSISTENT_CONV if kind == "conv" else PERSISTENT_DECONV)[key]
    ntiles = tiles[0] * tiles[1] * tiles[2]
    assert ntiles > resident, (ntiles, resident)
    per = R.ceil_div(ntiles, min(ntiles, resident))
    assert per >= 2 and (ntiles % per != 0 or R.ceil_div(ntiles, per) < min(ntiles, resident)), "a ragged last run or a block without work"
    shape = tiles_shape(kind, key, tiles)
    figs = Figures()
    seed = 400 + ntiles % 97
    if kind == "conv":
        cfg = conv_cfg(key)
        x, w, bias = conv_inputs(cfg, B, shape, seed)
        ref = refs(lambda f: R.conv(R.model_x(f, x), R.model_w(f, w), bias, key[3]), formats)
        for fmt in formats:
            judge(figs, fmt, run(lambda: run_conv(fmt, cfg, x, w, bias, device)), *ref[fmt], R.conv_products(cfg), (kind, key, fmt, shape))
    else:
        cfg = deconv_cfg(key)
        x, w, bias, skip = deconv_inputs(cfg, B, shape, seed)
        ref = refs(lambda f: R.deconv(R.model_x(f, x), R.model_w(f, w), bias, key[2], skip=R.model_x(f, skip)), formats)
        for fmt in formats:
            judge(figs, fmt, run(lambda: run_deconv(fmt, cfg, x, w, bias, skip, device)), *ref[fmt], R.deconv_products(cfg), (kind, key, fmt, shape))
        g = torch.Generator().manual_seed(seed + 1)
        pw, pb = torch.randn(8, generator=g), torch.randn(1, generator=g)
        logits, S1, A = prob_reference("bf16x3", cfg, x, w, bias, skip, pw, pb)
        judge_logits(figs, "bf16x3", run(lambda: run_prob("bf16x3", cfg, x, w, bias, skip, pw, pb, device)), logits, S1, R.deconv_products(cfg),
                     ("deconv3d_prob", key, shape))
    figs.close_bits()
    figs.show("persistent %s %s, %d tiles %s on %d blocks" % (kind, key, ntiles, shape, resident))
    return figs


# 4 = runs of 2 + 2 and a block that returns; 7 = 3 + 3 + 1; 10 = 4 + 4 + 2; the tiles lie along a different axis each time
EMULATOR_TILES = [(2, 2, 1), (7, 1, 1), (1, 2, 5)]


@pytest.mark.parametrize("tiles", EMULATOR_TILES, ids=lambda t: "%d_tiles" % (t[0] * t[1] * t[2]))
@pytest.mark.parametrize("kind,key", persistent_instantiations(), ids=flat_id)
def test_persistent_tile_loop(emu, kind, key, tiles):
    assert tiles[0] * tiles[1] * tiles[2] in (4, 7, 10)
    case_persistent(emu, kind, key, tiles, 2 if tiles == EMULATOR_TILES[0] else 1, EMULATOR_BLOCKS)


def test_every_persistent_instantiation_is_run():
    assert len(persistent_instantiations()) == 8 and sum(len(v) for v in PERSISTENT_CONV.values()) + sum(len(v) for v in PERSISTENT_DECONV.values()) == 23
    assert sorted(t[0] * t[1] * t[2] for t in EMULATOR_TILES) == [4, 7, 10]
