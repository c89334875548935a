"""TEST ORACLE: a float64 numpy restatement of the Gipuma-route fusion contract, written from the contract
text and not from the kernel.  Every decision carries a margin: a comparison is BORDERLINE when flipping it lies within the fp32
error bound of its operands (the rule of parity_cases.fusion_vs_fp64: margin under SAFETY times the bound).  The comparisons:
z > 0, the image bounds, the disparity test, and the floor(u + .5) / floor(u) choices (borderline only if the two candidate
texels lead to different decisions or different X_c).  The depth-range test compares fp32 map values with the bounds and is
exact on the device (the bounds are rounded inwards), so it has no margin.

    cams = cameras(cams_f32)                              # fp64 P, M^-1, C, f from the float32 file values
    out = fuse_view(r, depths, colors, cams, used_r, params, pixels=None)
    run = fuse_scene(depths, colors, cams, params)        # every view in order with the oracle's own used maps
"""
import numpy as np

U = 2.0 ** -24                    # fp32 unit roundoff
SAFETY = 16.0


def cameras(cams):
    """cams [N,2,4,4] float32 -> dict of fp64 arrays: P [N,3,4] = ([K 0; 0 1] E)[:3], M^-1 [N,3,3], C [N,3], f [N]."""
    cams = np.asarray(cams, np.float32)
    n = cams.shape[0]
    P = np.zeros((n, 3, 4))
    for v in range(n):
        k4 = np.zeros((4, 4))
        k4[:3, :3] = cams[v, 1, :3, :3]
        k4[3, 3] = 1.0
        P[v] = (k4 @ cams[v, 0].astype(np.float64))[:3]
    Minv = np.linalg.inv(P[:, :, :3])
    C = -np.einsum("nij,nj->ni", Minv, P[:, :, 3])
    return {"P": P, "Minv": Minv, "C": C, "f": cams[:, 1, 0, 0].astype(np.float64)}


def fuse_view(r, depths, colors, cams, used_r, params, pixels=None):
    """Reference view r with used[r] = used_r (bool [H,W]).  depths [N,H,W] float32 (filtered), colors [N,H,W,3] uint8.
    params: disp_thresh, num_consistent, depth_min, depth_max.  pixels: flat indices to evaluate (None = all).
    -> dict over the evaluated pixels `pix`: accepted (bool), border (bool), pos [k,3] fp64, rgb [k,3] int, n (int), and
    marks: list over other views c of (pixel index into pix, flat index into view c) of ACCEPTED pixels' marks, plus
    marks_border: the same for borderline pixels (both candidates of a borderline floor)."""
    N, H, W = depths.shape
    pix = np.arange(H * W) if pixels is None else np.asarray(pixels)
    x, y = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    d = depths[r].reshape(-1)[pix].astype(np.float64)
    lo, hi = params["depth_min"], params["depth_max"]
    thr = params["disp_thresh"]
    thr_err = abs(float(np.float32(thr)) - thr)
    active_all = (~used_r.reshape(-1)[pix]) & (d >= lo) & (d <= hi)
    if not active_all.all():                   # evaluate the active pixels only, then scatter back
        sub = fuse_view(r, depths, colors, cams, used_r, params, pixels=pix[active_all])
        k = len(pix)
        out = {"pix": pix, "accepted": np.zeros(k, bool), "border": np.zeros(k, bool), "pos": np.zeros((k, 3)),
               "rgb": np.zeros((k, 3), np.int64), "n": np.zeros(k, np.int64)}
        for key in ("accepted", "border", "pos", "rgb", "n"):
            out[key][active_all] = sub[key]
        idx = np.flatnonzero(active_all)
        out["marks"] = [(c, idx[i], flat) for c, i, flat in sub["marks"]]
        out["marks_border"] = sub["marks_border"]
        return out
    active = active_all
    dd = np.where(active, d, 0.0)
    P, Minv, C, f = cams["P"], cams["Minv"], cams["C"], cams["f"]
    # step 2: X = M_r^-1 ([x d, y d, d] - P_r[:, 3])
    q = np.stack([x * dd, y * dd, dd], -1) - P[r, :, 3]
    X = q @ Minv[r].T
    k = len(pix)
    sum_pos = X.copy()
    sum_rgb = colors[r].reshape(-1, 3)[pix].astype(np.int64)
    n = np.zeros(k, np.int64)
    border = np.zeros(k, bool)
    hits = []                                            # (c, mask over pix, flat mark index) of consistent views
    cand_mark = []
    for c in range(N):
        if c == r:
            continue
        Hm = P[c, :, :3] @ Minv[r]
        t = P[c, :, :3] @ C[r] + P[c, :, 3]
        proj = np.concatenate([X, np.ones((k, 1))], 1) @ P[c].T          # step 3, as the contract states it
        up, vp, z = proj[:, 0], proj[:, 1], proj[:, 2]
        # fp32 error bounds of the device's d * (H [x, y, 1]) + t
        mag = np.abs(dd)[:, None] * (np.abs(Hm[:, 0])[None] * x[:, None] + np.abs(Hm[:, 1])[None] * y[:, None] + np.abs(Hm[:, 2])[None]) + np.abs(t)[None]
        e_up, e_vp, e_z = 4 * U * mag[:, 0], 4 * U * mag[:, 1], 4 * U * mag[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = up / z, vp / z
            e_u = (e_up + np.abs(u) * e_z) / np.abs(z) + U * np.abs(u)
            e_v = (e_vp + np.abs(v) * e_z) / np.abs(z) + U * np.abs(v)
        S = SAFETY
        zpos = z > 0
        b_z = active & (np.abs(z) <= S * e_z)
        inb = zpos & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        b_in = active & zpos & ((np.abs(u) <= S * e_u) | (np.abs(u - W) <= S * e_u) | (np.abs(v) <= S * e_v) | (np.abs(v - H) <= S * e_v))
        go = active & inb
        fb = f[r] * np.linalg.norm(C[r] - C[c])
        uu, vv = np.where(go, u, 0.0), np.where(go, v, 0.0)

        def decide(ix, iy):
            ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
            dc = depths[c][iy, ix].astype(np.float64)
            inr = (dc >= lo) & (dc <= hi)
            with np.errstate(divide="ignore", invalid="ignore"):
                D = np.abs(fb / z - fb / dc)
                e_D = np.abs(fb / z) * (4 * U + e_z / np.abs(z)) + np.abs(fb / dc) * 3 * U
            ok = go & inr & (D < thr)
            b_D = go & inr & (np.abs(D - thr) <= S * e_D + thr_err)
            return ok, dc, b_D, iy * W + ix

        rx, ry = np.floor(uu + 0.5).astype(np.int64), np.floor(vv + 0.5).astype(np.int64)
        ok, dc, b_D, tex = decide(rx, ry)
        b_tex = np.zeros(k, bool)
        for axis in (0, 1):                               # the other texel of a near-half coordinate
            val = (uu if axis == 0 else vv) + 0.5
            err = (e_u if axis == 0 else e_v) + U * np.abs(val)
            frac = val - np.floor(val)
            near = go & (np.minimum(frac, 1 - frac) <= S * err)
            alt = np.where(frac < 0.5, -1, 1)
            ax, ay = (rx + alt, ry) if axis == 0 else (rx, ry + alt)
            ok2, dc2, _, tex2 = decide(ax, ay)
            col1, col2 = colors[c].reshape(-1, 3)[tex], colors[c].reshape(-1, 3)[tex2]
            diff = (ok2 != ok) | (ok & ((dc2 != dc) | (col1 != col2).any(1)))
            b_tex |= near & diff
        iu, iv = np.floor(uu).astype(np.int64), np.floor(vv).astype(np.int64)
        b_floor = np.zeros(k, bool)
        for val, err in ((uu, e_u), (vv, e_v)):
            frac = val - np.floor(val)
            b_floor |= go & ok & (np.minimum(frac, 1 - frac) <= S * err)
        border |= b_z | b_in | b_D | b_tex | b_floor
        # X_c = back-projection of view c at (floor(u), floor(v)) with depth d_c
        qc = np.stack([iu * dc, iv * dc, dc], -1) - P[c, :, 3]
        with np.errstate(invalid="ignore"):
            Xc = qc @ Minv[c].T
        sum_pos[ok] += Xc[ok]
        sum_rgb[ok] += colors[c].reshape(-1, 3)[tex[ok]]
        n += ok
        iu_c, iv_c = np.clip(iu, 0, W - 1), np.clip(iv, 0, H - 1)
        hits.append((c, ok, iv_c * W + iu_c))
        # a borderline floor may mark either neighbour: both are uncertain
        cand_mark.append((c, go & (ok | b_D | b_tex), iv_c, iu_c))
    accepted = active & (n >= params["num_consistent"])
    pos = sum_pos / (n + 1)[:, None]
    rgb = sum_rgb // (n + 1)[:, None]
    marks, marks_border = [], []
    for c, ok, flat in hits:
        sel = accepted & ok & ~border
        marks.append((c, np.flatnonzero(sel), flat[sel]))
    for c, cand, iv_c, iu_c in cand_mark:
        sel = border & cand
        idx = np.flatnonzero(sel)
        cells = set()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cells.add(((np.clip(iv_c[sel] + dy, 0, H - 1)) * W + np.clip(iu_c[sel] + dx, 0, W - 1)).tobytes())
        flats = np.unique(np.concatenate([np.frombuffer(b, np.int64) for b in cells])) if idx.size else np.zeros(0, np.int64)
        marks_border.append((c, flats))
    return {"pix": pix, "accepted": accepted, "border": border & active, "pos": pos, "rgb": rgb, "n": n,
            "marks": marks, "marks_border": marks_border}


def fuse_scene(depths, colors, cams, params):
    """Every view as reference view, in order, with the oracle's own used maps.  -> (per-view results, final used [N,H,W] bool)."""
    N, H, W = depths.shape
    used = np.zeros((N, H, W), bool)
    outs = []
    for r in range(N):
        o = fuse_view(r, depths, colors, cams, used[r].copy(), params)
        for c, _, flat in o["marks"]:
            used[c].reshape(-1)[flat] = True
        o["skipped"] = used[r].copy()
        outs.append(o)
    return outs, used
