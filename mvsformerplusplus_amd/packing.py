"""Host-side parameter preparation for the HIP kernels: BatchNorm folding and MFMA weight packing.

Packed conv layout (read by ``conv3d_mfma_kernel``; DESIGN.md "MFMA weight packing"):

    K-quads are enumerated per channel chunk ("pass", CH input channels) tap-major:
        kq = tap * (CH/4) + cq,   tap = (kd*3 + kh)*3 + kw,   cq = channel quad inside the chunk
    and consumed four at a time ("step"); lane group g = lane >> 4 of the wave owns quad 4*step + g.
    packed[pass][step][mb][lane = g*16 + j][s] = W'[cout = 16*mb + j][cin = pass*CH + 4*cq + s][tap]
    (zero where the quad index or cout runs past the end).  W' = W * gamma / sqrt(var + eps).

Packed deconv layout (``deconv3d_mfma_kernel``): all 27 taps, 16-channel blocks q:
    packed[tap][q][mb][lane = g*16 + j][s] = Wt'[cin = 16*q + 4*g + s][cout = 16*mb + j][tap]
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

BN_EPS = 1e-5


def fold_bn(weight: torch.Tensor, bn: Dict[str, torch.Tensor], out_dim: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fold eval-mode BatchNorm into the preceding bias-free conv.  ``out_dim`` = axis of ``weight`` that is Cout."""
    scale = bn["weight"].double() / torch.sqrt(bn["running_var"].double() + float(bn.get("eps", BN_EPS)))
    shift = bn["bias"].double() - bn["running_mean"].double() * scale
    shape = [1] * weight.dim()
    shape[out_dim] = -1
    return (weight.double() * scale.reshape(shape)).float(), shift.float()


def conv_chunk(cin: int, stride: Tuple[int, int, int]) -> int:
    """Channel chunk staged per LDS pass - must match the ConvCfg table in csrc/conv_kernels.hip."""
    return 16 if tuple(stride) == (1, 1, 1) and cin >= 16 else 8


def pack_conv_weights(w: torch.Tensor, ch: int) -> torch.Tensor:
    """w [Cout, Cin, kd, 3, 3] (BN already folded) -> packed fp32 1-D tensor."""
    cout, cin = w.shape[:2]
    ntap = w.shape[2] * w.shape[3] * w.shape[4]
    assert cin % ch == 0 and ch % 4 == 0
    qc = ch // 4
    npass = cin // ch
    nquad = ntap * qc
    nstep = (nquad + 3) // 4
    mrep = (cout + 15) // 16
    wt = w.reshape(cout, npass, qc, 4, ntap).float()                       # [co, pass, cq, s, tap]
    wt = wt.permute(1, 4, 2, 0, 3).reshape(npass, nquad, cout, 4)          # [pass, kq = tap*qc + cq, co, s]
    full = torch.zeros(npass, nstep * 4, mrep * 16, 4, dtype=torch.float32, device=w.device)
    full[:, :nquad, :cout] = wt
    full = full.reshape(npass, nstep, 4, mrep, 16, 4)                      # [pass, step, g, mb, j, s]
    return full.permute(0, 1, 3, 2, 4, 5).contiguous().reshape(-1)         # [pass, step, mb, g, j, s]


def pack_deconv_weights(w: torch.Tensor) -> torch.Tensor:
    """w [Cin, Cout, 3, 3, 3] (ConvTranspose3d layout, BN folded over Cout) -> packed fp32 1-D tensor."""
    cin, cout = w.shape[:2]
    assert cin % 16 == 0 and tuple(w.shape[2:]) == (3, 3, 3)
    nq = cin // 16
    mrep = (cout + 15) // 16
    wt = w.reshape(nq, 4, 4, cout, 27).float()                             # [q, g, s, co, tap]
    full = torch.zeros(nq, 4, 4, mrep * 16, 27, dtype=torch.float32, device=w.device)
    full[:, :, :, :cout] = wt
    full = full.reshape(nq, 4, 4, mrep, 16, 27)                            # [q, g, s, mb, j, tap]
    return full.permute(5, 0, 3, 1, 4, 2).contiguous().reshape(-1)         # [tap, q, mb, g, j, s]


def split_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 [...] -> bf16 [2, ...] with x ~= hi + lo (both round-to-nearest-even), the operand format of the bf16x3 kernels: the host
    mirror of split_bf16 / split_bf16_bits in csrc/split_format.h, whose header states the whole contract."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo])


def _split_f16(x: torch.Tensor) -> torch.Tensor:
    """fp32 [...] -> fp16 [2, ...] with x ~= hi + lo (22 significant bits; lo flushes below 6e-8): operands of the f16x2 kernels,
    viewed as bf16 so that the packers below stay dtype-agnostic (2-byte elements, bit pattern preserved)."""
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return torch.stack([hi, lo]).view(torch.bfloat16)


def f16x2(packer, *args):
    """One of the pack_*_bf16x3 functions with the fp16 hi + lo split instead of the bf16 one (the weights of MVS_PREC_F16X2)."""
    return packer(*args, split=_split_f16)


def pack_conv_weights_bf16x3(w: torch.Tensor, ch: int, split=None) -> torch.Tensor:
    """w [Cout, Cin, kd, 3, 3] (BN folded) -> bf16 1-D tensor for ``conv3d_mfma_bf16x3_kernel``:

        packed[pass][step][mb][hi|lo][lane = g*16 + j][e] = W'[16*mb + j][pass*CH + 8*oc + e][tap],
        (tap, oc) = divmod(4*step + g, CH/8)      (channel octets enumerated tap-major, four per step)
    """
    cout, cin = w.shape[:2]
    ntap = w.shape[2] * w.shape[3] * w.shape[4]
    assert cin % ch == 0 and ch % 8 == 0
    opt = ch // 8
    npass = cin // ch
    noct = ntap * opt
    nstep = (noct + 3) // 4
    mrep = (cout + 15) // 16
    wt = w.reshape(cout, npass, opt, 8, ntap).float().permute(1, 4, 2, 0, 3).reshape(npass, noct, cout, 8)   # [pass, o, co, e]
    full = torch.zeros(npass, nstep * 4, mrep * 16, 8, dtype=torch.float32, device=w.device)
    full[:, :noct, :cout] = wt
    full = full.reshape(npass, nstep, 4, mrep, 16, 8).permute(0, 1, 3, 2, 4, 5)                              # [pass, step, mb, g, j, e]
    return (split or split_bf16)(full).permute(1, 2, 3, 0, 4, 5, 6).contiguous().reshape(-1)                           # [pass, step, mb, 2, g, j, e]


def fpn_chunk(cin: int, stride: int) -> int:
    """Input channels staged per LDS pass by ``conv2d_split_kernel`` (csrc/conv2d_split.h Conv2dShape::CH): all of them up to 32 at stride 1,
    one octet at stride 2 (the 2x wider staged tile).  Cin is first padded to a multiple of 8."""
    cinp = (cin + 7) // 8 * 8
    return min(cinp, 32) if stride == 1 else 8


def pack_fpn_conv_weights(w: torch.Tensor, stride: int) -> torch.Tensor:
    """Conv2d weight [Cout, Cin, k, k] (BN folded) -> the bf16x3 packing of ``conv2d_split_kernel``: Cin zero-padded to a multiple of 8,
    taps (ky*k + kx) enumerated like the 3-D packer's with kd = 1."""
    cout, cin = w.shape[:2]
    cinp = (cin + 7) // 8 * 8
    if cinp != cin:
        w = torch.cat([w.float(), w.new_zeros(cout, cinp - cin, *w.shape[2:]).float()], 1)
    return pack_conv_weights_bf16x3(w.float().unsqueeze(2), fpn_chunk(cin, stride))


def fpn_enc_dgrad_class_taps(w: torch.Tensor) -> torch.Tensor:
    """The four parity classes of a stride-2 layer's data gradient: w [Cout, Cin, k, k] (k = 3 | 5, padding k // 2)
    -> [4, Cin, Cout, 3, 3], class 2 py + px.  Row 2 i + py of dx takes tap ky from row o = i + r - 1 of dz with ky = py + k // 2 + 2 - 2 r
    (r = 0, 1, 2; a ky outside 0 .. k - 1 is a zero tap), and the same along x: each class is a 3x3 stride-1 padding-1 correlation of dz."""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    assert w.shape[3] == k and k in (3, 5), tuple(w.shape)
    wt = w.float().transpose(0, 1)                                               # [Cin, Cout, k, k]
    out = wt.new_zeros(4, cin, cout, 3, 3)
    for py in range(2):
        for px in range(2):
            for r in range(3):
                ky = py + k // 2 + 2 - 2 * r
                for s in range(3):
                    kx = px + k // 2 + 2 - 2 * s
                    if 0 <= ky < k and 0 <= kx < k:
                        out[2 * py + px, :, :, r, s] = wt[:, :, ky, kx]
    return out


def pack_fpn_enc_dgrad_weights(w: torch.Tensor) -> torch.Tensor:
    """Stride-2 layer weight [Cout, Cin, k, k] -> the four classes' ``pack_fpn_conv_weights(.., 1)`` one after the other
    (``mvs_fpn_enc_dgrad``)."""
    return torch.cat([pack_fpn_conv_weights(c.contiguous(), 1) for c in fpn_enc_dgrad_class_taps(w)])


def pack_linear_bf16x3(w: torch.Tensor, split=None) -> torch.Tensor:
    """w [N, K] (y = x @ w.T; N % 16 == 0, K % 32 == 0) -> bf16 1-D tensor for ``tr_gemm_kernel``:

        packed[step][mb][hi|lo][lane = g*16 + j][e] = w[16*mb + j][32*step + 8*g + e]
    """
    n, k = w.shape
    assert n % 16 == 0 and k % 32 == 0, (n, k)
    full = w.float().reshape(n // 16, 16, k // 32, 4, 8).permute(2, 0, 3, 1, 4)                                # [step, mb, g, j, e]
    return (split or split_bf16)(full).permute(1, 2, 0, 3, 4, 5).contiguous().reshape(-1)                                # [step, mb, 2, g, j, e]


def patch_embed_matrix(w: torch.Tensor) -> torch.Tensor:
    """Conv3d(kernel = stride) weight [Cout, Cin, rd, rh, rw] -> [Cout, patch_voxel*Cin + ci] (k order of the patch gather)."""
    co, ci = w.shape[:2]
    return w.float().permute(0, 2, 3, 4, 1).reshape(co, -1).contiguous()


def patch_expand_matrix(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose3d(kernel = stride) weight [Cin, Cout, rd, rh, rw] -> [patch_voxel*Cout + co, Cin]."""
    ci, co = w.shape[:2]
    return w.float().permute(2, 3, 4, 1, 0).reshape(-1, ci).contiguous()


def deconv_class_taps(sd: int):
    """Parity classes of ConvTranspose3d(k3, stride (sd,2,2)) in the kernels' order, each a list of tap indices
    (kd*3 + kh)*3 + kw ordered (a_d, a_h, a_w) with a_w fastest - mirrors ``bf_deconv_load_step``."""
    out = []
    for cls in range((2 if sd == 2 else 1) * 4):
        pw, ph, pd = cls & 1, (cls >> 1) & 1, (cls >> 2) if sd == 2 else 0
        kds = ([0, 2] if pd else [1]) if sd == 2 else [0, 1, 2]
        khs = [0, 2] if ph else [1]
        kws = [0, 2] if pw else [1]
        out.append([(kd * 3 + kh) * 3 + kw for kd in kds for kh in khs for kw in kws])
    return out


def pack_deconv_weights_bf16x3(w: torch.Tensor, sd: int, split=None) -> torch.Tensor:
    """w [Cin, Cout, 3, 3, 3] (BN folded over Cout) -> bf16 1-D tensor for ``deconv3d_mfma_bf16x3_kernel``: per parity
    class, packed[step][mb][hi|lo][lane = g*16 + j][e] = Wt'[8*oc + e][16*mb + j][taps[ti]], (ti, oc) = divmod(4*step + g, Cin/8)."""
    cin, cout = w.shape[:2]
    assert cin % 8 == 0 and tuple(w.shape[2:]) == (3, 3, 3)
    opt = cin // 8
    mrep = (cout + 15) // 16
    wf = w.reshape(opt, 8, cout, 27).float()                                       # [oc, e, co, tap]
    chunks = []
    if cout == 8:
        # Cout = 8 fills only half of the 16 MFMA rows: the two x-parity classes of a (pd, ph) pair share their input voxels
        # (pw = 1 reads inputs mx+1 and mx with kw = 0 and 2, pw = 0 reads input mx with kw = 1), so rows 0-7 carry pw = 0
        # (zero weights on the mx+1 tap) and rows 8-15 pw = 1: 2 tap units per pair instead of 1 + 2, all 16 rows useful,
        # and one lane group pair stores the 64 contiguous bytes of the two output voxels 2mx, 2mx+1.
        classes = deconv_class_taps(sd)
        for c2 in range(len(classes) // 2):
            taps1 = classes[2 * c2 + 1]                                            # pw = 1: (a_d, a_h, a_w) with a_w fastest, kw in (0, 2)
            noct = len(taps1) * opt
            nst = (noct + 3) // 4
            full = torch.zeros(nst * 4, 16, 8, dtype=torch.float32, device=w.device)
            for ti, t1 in enumerate(taps1):
                kw = t1 % 3
                full[ti * opt:(ti + 1) * opt, 8:16] = wf[:, :, :, t1].permute(0, 2, 1)           # [oc, co, e]
                if kw == 2:                                                                       # input mx: pw = 0 uses kw = 1 of the same (kd, kh)
                    full[ti * opt:(ti + 1) * opt, 0:8] = wf[:, :, :, t1 - 1].permute(0, 2, 1)
            full = full.reshape(nst, 4, 1, 16, 8).permute(0, 2, 1, 3, 4)
            chunks.append((split or split_bf16)(full).permute(1, 2, 0, 3, 4, 5).contiguous().reshape(-1))
        return torch.cat(chunks)
    for taps in deconv_class_taps(sd):
        noct = len(taps) * opt
        nst = (noct + 3) // 4
        sel = wf[:, :, :, taps].permute(3, 0, 2, 1).reshape(noct, cout, 8)         # [o = ti*opt + oc, co, e]
        full = torch.zeros(nst * 4, mrep * 16, 8, dtype=torch.float32, device=w.device)
        full[:noct, :cout] = sel
        full = full.reshape(nst, 4, mrep, 16, 8).permute(0, 2, 1, 3, 4)             # [step, mb, g, j, e]
        chunks.append((split or split_bf16)(full).permute(1, 2, 0, 3, 4, 5).contiguous().reshape(-1))   # [step, mb, 2, g, j, e]
    return torch.cat(chunks)


def pad_bias(b: torch.Tensor) -> torch.Tensor:
    n = max(16, ((b.numel() + 15) // 16) * 16)
    out = torch.zeros(n, dtype=torch.float32, device=b.device)
    out[: b.numel()] = b.float()
    return out


def pack_generic_conv_weights(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv3d weight [Cout, Cin, kd, kh, kw] (BN already folded) -> [kd*kh*kw][Cin][Cout] fp32 (mvs_conv3d_generic_fwd)."""
    cout, cin = w.shape[:2]
    return w.float().permute(2, 3, 4, 1, 0).reshape(-1, cin, cout).contiguous()


def pack_generic_deconv_weights(w: torch.Tensor) -> torch.Tensor:
    """nn.ConvTranspose3d weight [Cin, Cout, kd, kh, kw] (BN folded along dim 1) -> [kd*kh*kw][Cin][Cout] fp32, taps NOT flipped
    (the kernel gathers input i = (o + p - k) / s for kernel index k)."""
    cin, cout = w.shape[:2]
    return w.float().permute(2, 3, 4, 0, 1).reshape(-1, cin, cout).contiguous()


def pack_fmt_linear(w: torch.Tensor) -> torch.Tensor:
    """w [N, K] (y = w @ x; N padded to a multiple of 16, K % 32 == 0) -> bf16 1-D tensor for the GEMMs of csrc/fmt_kernels.hip, whose
    operand is the previous GEMM's accumulator: k-slot (step, g, e) holds input channel 32*step + 16*(e >> 2) + 4*g + (e & 3):

        packed[step][mb][hi|lo][lane = g*16 + j][e] = w[16*mb + j][32*step + 16*(e >> 2) + 4*g + (e & 3)]
    """
    n, k = w.shape
    assert k % 32 == 0, (n, k)
    npad = (n + 15) // 16 * 16
    if npad != n:
        w = torch.cat([w.float(), w.new_zeros(npad - n, k).float()], 0)
    full = w.float().reshape(npad // 16, 16, k // 32, 2, 4, 4).permute(2, 0, 4, 1, 3, 5).reshape(k // 32, npad // 16, 4, 16, 8)  # [step, mb, g, j, e]
    return split_bf16(full).permute(1, 2, 0, 3, 4, 5).contiguous().reshape(-1)                                    # [step, mb, 2, g, j, e]


FMT_VECTORS = ("norm1.weight", "norm1.bias", "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.bias", "mlp.fc2.bias",
               "ls2.gamma")


def pack_fmt_block(sd: Dict[str, torch.Tensor], device="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    """One CrossBlock of the FMT (keys relative to ``FMT.layers.N.``; d_model 64, hidden 256) -> (packed weights bf16: q_proj | proj | fc1 |
    fc2 | [k_proj; v_proj], vectors fp32 [768] in the order of FMT_VECTORS): the layout constants FT_W_* / FT_V_* of fmt_kernels.hip.
    Packed on the host by default; device=None packs where the parameters live (plain tensor ops: a training step copies nothing to
    the host and does not synchronise) and gives the same bits."""
    mats = [sd["attn.q_proj.weight"], sd["attn.proj.weight"], sd["mlp.fc1.weight"], sd["mlp.fc2.weight"],
            torch.cat([sd["attn.k_proj.weight"], sd["attn.v_proj.weight"]], 0)]
    want = [(64, 64), (64, 64), (256, 64), (64, 256), (128, 64)]
    assert [tuple(m.shape) for m in mats] == want, [tuple(m.shape) for m in mats]
    f32 = (lambda t: t.detach().float()) if device is None else (lambda t: t.detach().float().to(device))
    w = torch.cat([pack_fmt_linear(f32(m)) for m in mats])
    v = torch.cat([f32(sd[k]).reshape(-1) for k in FMT_VECTORS])
    assert w.numel() == 12288 * 8 and v.numel() == 768
    return w, v


# ---- CrossVITDecoder (csrc/vitdec_kernels.hip) ----------------------------------------------------------
def pack_tokens_split(x: torch.Tensor) -> torch.Tensor:
    """x [M, C] fp32 (C % 32 == 0) -> the PACKED-SPLIT row operand of the vitdec GEMMs as a bf16 1-D tensor, rows zero-padded to a
    multiple of 16:  packed[row >> 4][k >> 5][hi|lo][lane = ((k >> 3) & 3) * 16 + (row & 15)][k & 7].  The kernels write this layout
    themselves; this host form is for tests and tools."""
    m, c = x.shape
    assert c % 32 == 0, (m, c)
    mp = (m + 15) // 16 * 16
    full = torch.zeros(mp, c, dtype=torch.float32, device=x.device)
    full[:m] = x.float()
    full = full.reshape(mp // 16, 16, c // 32, 4, 8).permute(0, 2, 3, 1, 4)                                       # [rb, step, g, li, e]
    return split_bf16(full).permute(1, 2, 0, 3, 4, 5).contiguous().reshape(-1)                                   # [rb, step, 2, g, li, e]


def unpack_tokens_split(p: torch.Tensor, m: int, c: int) -> torch.Tensor:
    """The inverse of pack_tokens_split (hi + lo in fp32) -> [m, c]; p may be the uint8 buffer a kernel wrote."""
    if p.dtype == torch.uint8:
        p = p.view(torch.bfloat16)
    mp = (m + 15) // 16 * 16
    f = p.float().reshape(mp // 16, c // 32, 2, 4, 16, 8)
    return (f[:, :, 0] + f[:, :, 1]).permute(0, 3, 1, 2, 4).reshape(mp, c)[:m].contiguous()


VITDEC_VECTORS = ("norm1.weight", "norm1.bias", "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.bias", "mlp.fc2.bias",
                  "ls2.gamma")


def pack_vitdec_block(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """One CrossBlock at d_model 768 (keys relative to the block) -> {"q", "kv" ([k_proj; v_proj]), "proj", "fc1", "fc2"}: each
    pack_linear_bf16x3, plus the fp32 vectors of VITDEC_VECTORS under their own names."""
    mats = {"q": sd["attn.q_proj.weight"], "kv": torch.cat([sd["attn.k_proj.weight"], sd["attn.v_proj.weight"]], 0),
            "proj": sd["attn.proj.weight"], "fc1": sd["mlp.fc1.weight"], "fc2": sd["mlp.fc2.weight"]}
    want = {"q": (768, 768), "kv": (1536, 768), "proj": (768, 768), "fc1": (3072, 768), "fc2": (768, 3072)}
    assert {k: tuple(v.shape) for k, v in mats.items()} == want, {k: tuple(v.shape) for k, v in mats.items()}
    out = {k: pack_linear_bf16x3(v.detach().float().cpu()) for k, v in mats.items()}
    for k in VITDEC_VECTORS:
        out[k] = sd[k].detach().float().cpu().reshape(-1).contiguous()
    return out


def pack_vitdec_block_train(sd: Dict[str, torch.Tensor], transposed: bool = True) -> Dict[str, torch.Tensor]:
    """pack_vitdec_block for a training step: packed WHERE THE PARAMETERS LIVE (plain tensor ops: no host copy,
    no synchronisation; the same bits as the host form), from the values they hold now - never cached, an optimiser updates them in
    place - plus, with `transposed`, "qT" / "kvT" / "projT" / "fc1T" / "fc2T" = pack_linear_bf16x3 of the transposed weights, the
    operands of the data gradients dX = dY W."""
    f32 = lambda t: t.detach().float()
    mats = {"q": f32(sd["attn.q_proj.weight"]), "kv": torch.cat([f32(sd["attn.k_proj.weight"]), f32(sd["attn.v_proj.weight"])], 0),
            "proj": f32(sd["attn.proj.weight"]), "fc1": f32(sd["mlp.fc1.weight"]), "fc2": f32(sd["mlp.fc2.weight"])}
    want = {"q": (768, 768), "kv": (1536, 768), "proj": (768, 768), "fc1": (3072, 768), "fc2": (768, 3072)}
    assert {k: tuple(v.shape) for k, v in mats.items()} == want, {k: tuple(v.shape) for k, v in mats.items()}
    out = {k: pack_linear_bf16x3(v) for k, v in mats.items()}
    if transposed:
        out.update({k + "T": pack_linear_bf16x3(v.t()) for k, v in mats.items()})
    for k in VITDEC_VECTORS:
        out[k] = f32(sd[k]).reshape(-1).contiguous()
    return out


def _fold_conv_bn(w: torch.Tensor, b: torch.Tensor, bn: Dict[str, torch.Tensor], out_dim: int):
    """Conv (with bias) + eval BatchNorm -> (w * scale, (b - mean) * scale + beta), computed in fp64."""
    scale = bn["weight"].double() / torch.sqrt(bn["running_var"].double() + float(bn.get("eps", BN_EPS)))
    shape = [1] * w.dim()
    shape[out_dim] = -1
    return (w.double() * scale.reshape(shape)).float(), ((b.double() - bn["running_mean"].double()) * scale + bn["bias"].double()).float()


def pack_vitdec_conv(w: torch.Tensor, b: torch.Tensor, bn: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """proj: Conv2d weight [Cout, Cin, 3, 3] + bias + BatchNorm -> (pack_linear_bf16x3 of the [Cout, 9 Cin] matrix whose column is
    (ky * 3 + kx) * Cin + c, folded bias [Cout])."""
    wf, bf = _fold_conv_bn(w.detach().float().cpu(), b.detach().float().cpu(), {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in bn.items()}, 0)
    cout, cin = wf.shape[:2]
    assert cout % 128 == 0 and cin % 64 == 0 and tuple(wf.shape[2:]) == (3, 3), tuple(wf.shape)
    return pack_linear_bf16x3(wf.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()), bf.contiguous()


def pack_vitdec_deconv(w: torch.Tensor, b: torch.Tensor, bn: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """upsampler: ConvTranspose2d(4, stride 2, padding 1) weight [Cin, Cout, 4, 4] + bias + BatchNorm -> (the four parity classes
    cls = 2 py + px one after the other, each pack_linear_bf16x3 of the [Cout padded to 128, 4 Cin] matrix whose column is
    (2 ay + ax) * Cin + c and holds w[c][co][1 - py + 2 ay][1 - px + 2 ax] - output (2 y + py, 2 x + px) reads input (y + py - ay,
    x + px - ax) -, folded bias [Cout])."""
    wf, bf = _fold_conv_bn(w.detach().float().cpu(), b.detach().float().cpu(), {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in bn.items()}, 1)
    cin, cout = wf.shape[:2]
    assert cin % 64 == 0 and cout % 4 == 0 and tuple(wf.shape[2:]) == (4, 4), tuple(wf.shape)
    npad = (cout + 127) // 128 * 128
    chunks = []
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        m = torch.zeros(npad, 4, cin, dtype=torch.float32)
        for ay in range(2):
            for ax in range(2):
                m[:cout, 2 * ay + ax] = wf[:, :, 1 - py + 2 * ay, 1 - px + 2 * ax].t()
        chunks.append(pack_linear_bf16x3(m.reshape(npad, 4 * cin)))
    return torch.cat(chunks), bf.contiguous()


VITDEC_HEAD = ("proj", "upsampler0", "upsampler1")


def pack_vitdec_head_train(sd: Dict[str, torch.Tensor], transposed: bool = True, forward: bool = True) -> Dict[str, Dict[str, torch.Tensor]]:
    """The head's convolution weights for a training step (keys relative to the decoder: "proj.0.weight",
    "upsampler0.0.weight", "upsampler1.0.weight", any subset), packed WHERE THE PARAMETERS LIVE from the values they hold now (plain
    tensor ops, never cached) -> per layer {"w": the forward operand, the bits pack_vitdec_conv / pack_vitdec_deconv give for an
    identity BatchNorm} and, with `transposed`, "wT": the data gradient's.  proj's "wT" is pack_linear_bf16x3 of [768, 9 x 256] with
    column (3 ky + kx) 256 + co = w[co][c][2 - ky][2 - kx] (flipped, channel-transposed taps); an upsampler's is pack_linear_bf16x3 of
    [Cin, 16 Cout] with column (4 ky + kx) Cout + co = w[c][co][ky][kx]: input token (y, x) reads the fine map at (2 y - 1 + ky,
    2 x - 1 + kx)."""
    out = {}
    for name in VITDEC_HEAD:
        if name + ".0.weight" not in sd:
            continue
        w = sd[name + ".0.weight"].detach().float()
        if name == "proj":
            cout, cin = w.shape[:2]
            assert cout % 128 == 0 and cin % 128 == 0 and tuple(w.shape[2:]) == (3, 3), tuple(w.shape)
            out[name] = {"w": pack_linear_bf16x3(w.permute(0, 2, 3, 1).reshape(cout, 9 * cin))} if forward else {}
            if transposed:
                out[name]["wT"] = pack_linear_bf16x3(w.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, 9 * cout))
            continue
        cin, cout = w.shape[:2]
        assert cin % 128 == 0 and cout % 64 == 0 and tuple(w.shape[2:]) == (4, 4), tuple(w.shape)
        npad = (cout + 127) // 128 * 128
        chunks = []
        for cls in range(4 if forward else 0):
            py, px = cls >> 1, cls & 1
            m = w.new_zeros(npad, 4, cin)
            for ay in range(2):
                for ax in range(2):
                    m[:cout, 2 * ay + ax] = w[:, :, 1 - py + 2 * ay, 1 - px + 2 * ax].t()
            chunks.append(pack_linear_bf16x3(m.reshape(npad, 4 * cin)))
        out[name] = {"w": torch.cat(chunks)} if forward else {}
        if transposed:
            out[name]["wT"] = pack_linear_bf16x3(w.permute(0, 2, 3, 1).reshape(cin, 16 * cout))
    return out


# ---- DINOv2 ViT-B/14 backbone (csrc/vitdec_kernels.hip, csrc/vit_attention_kernels.hip) ----------------------
VIT_VECTORS = ("norm1.weight", "norm1.bias", "attn.qkv.bias", "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.bias",
               "mlp.fc2.bias", "ls2.gamma")
VIT_PATCH_K, VIT_PATCH_KPAD = 588, 640


def pack_vit_block(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """One DINOv2 block at embed_dim 768 (keys relative to the block) -> {"qkv" ([2304, 768]: q | k | v, 12 heads of 64 each), "proj", "fc1",
    "fc2"}: each pack_linear_bf16x3, plus the fp32 vectors of VIT_VECTORS under their own names."""
    mats = {"qkv": sd["attn.qkv.weight"], "proj": sd["attn.proj.weight"], "fc1": sd["mlp.fc1.weight"], "fc2": sd["mlp.fc2.weight"]}
    want = {"qkv": (2304, 768), "proj": (768, 768), "fc1": (3072, 768), "fc2": (768, 3072)}
    assert {k: tuple(v.shape) for k, v in mats.items()} == want, {k: tuple(v.shape) for k, v in mats.items()}
    out = {k: pack_linear_bf16x3(v.detach().float().cpu()) for k, v in mats.items()}
    for k in VIT_VECTORS:
        out[k] = sd[k].detach().float().cpu().reshape(-1).contiguous()
    return out


def pack_vit_patch_embed(w: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """patch_embed.proj: Conv2d(3, 768, 14, stride 14) weight [768, 3, 14, 14] + bias -> (pack_linear_bf16x3 of the [768, 640] matrix
    whose column is c * 196 + ky * 14 + kx, columns 588 .. 639 zero: the GEMM's K granularity is 64; bias fp32 [768])."""
    assert tuple(w.shape) == (768, 3, 14, 14) and tuple(b.shape) == (768,), (tuple(w.shape), tuple(b.shape))
    m = torch.zeros(768, VIT_PATCH_KPAD, dtype=torch.float32)
    m[:, :VIT_PATCH_K] = w.detach().float().cpu().reshape(768, VIT_PATCH_K)
    return pack_linear_bf16x3(m), b.detach().float().cpu().contiguous()


def vit_position_table(pos_embed: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """The position rows of a gh x gw patch grid, fp32 [gh gw + 1, 768], by the reference's recipe (dinov2.py interpolate_pos_encoding):
    row 0 is the class position; the side x side patch table is resized with bicubic F.interpolate called with
    scale_factor = ((gh + 0.1) / side, (gw + 0.1) / side) - PyTorch maps coordinates with the GIVEN factors, so the same function is
    called with the same arguments here, nothing is re-derived.  The first factor belongs to the rows of the grid (the image's height,
    which the reference names `w`).  A square grid of the table's own size returns the table as it is.  Parameter preprocessing:
    computed once per (grid, parameter version) and cached by the module."""
    import math
    import torch.nn.functional as F
    p = pos_embed.detach().float().cpu()
    N, dim = p.shape[1] - 1, p.shape[2]
    if gh * gw == N and gh == gw:
        return p[0].contiguous()
    side = int(math.sqrt(N))
    assert side * side == N, N
    grid = p[:, 1:].reshape(1, side, side, dim).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, scale_factor=((gh + 0.1) / math.sqrt(N), (gw + 0.1) / math.sqrt(N)), mode="bicubic")
    assert tuple(grid.shape[-2:]) == (gh, gw), (tuple(grid.shape), gh, gw)
    return torch.cat((p[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, dim)), 0).contiguous()


def pack_vit_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, npad: int) -> torch.Tensor:
    """q, k, v [NV, 12, ntok, 64] fp32 (q already multiplied by scale * log2(e)) -> the operand buffer of the attention core as a uint8
    1-D tensor: per (view, head) q | k as pack_tokens_split rows (zero-padded to npad, a multiple of 32), then v transposed:
    vt[key >> 5][d >> 4][hi|lo][lane = g * 16 + (d & 15)][e] with key & 31 = 16 (e >> 2) + 4 g + (e & 3).  The qkv projection's epilogue
    writes this layout itself; this host form is for tests and tools."""
    NV, H, ntok, D = q.shape
    assert H == 12 and D == 64 and npad % 32 == 0 and npad >= ntok and k.shape == q.shape and v.shape == q.shape, (tuple(q.shape), npad)
    parts = []
    for view in range(NV):
        for h in range(H):
            parts.append(pack_tokens_split(torch.cat([q[view, h].float(), q.new_zeros(npad - ntok, D).float()])))
            parts.append(pack_tokens_split(torch.cat([k[view, h].float(), k.new_zeros(npad - ntok, D).float()])))
            vp = torch.cat([v[view, h].float(), v.new_zeros(npad - ntok, D).float()])
            vt = vp.reshape(npad // 32, 2, 4, 4, 4, 16).permute(0, 4, 2, 5, 1, 3).reshape(npad // 32, 4, 4, 16, 8)   # [ks, db, g, d & 15, e]
            parts.append(split_bf16(vt).permute(1, 2, 0, 3, 4, 5).contiguous().reshape(-1))                       # [ks, db, 2, g, d, e]
    return torch.cat(parts).view(torch.uint8)
