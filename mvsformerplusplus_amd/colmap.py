"""COLMAP sparse models: readers and writers for the binary and text formats, and the camera matrices colmap2mvsnet.py derives
from them.

The reference (`colmap2mvsnet.py:15-261`, COLMAP's read_model.py) builds one namedtuple per image and per point and unpacks every
observation with `struct`.  Here the per-image `points2D` and the per-point tracks are read as whole numpy arrays; only the
records themselves (one per image, one per point) are walked in Python.  Images keep their file order, as the reference's dict.
"""
from __future__ import annotations

import collections
import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

CameraModel = collections.namedtuple("CameraModel", ["model_id", "model_name", "num_params"])
CAMERA_MODELS = [
    CameraModel(0, "SIMPLE_PINHOLE", 3), CameraModel(1, "PINHOLE", 4), CameraModel(2, "SIMPLE_RADIAL", 4),
    CameraModel(3, "RADIAL", 5), CameraModel(4, "OPENCV", 8), CameraModel(5, "OPENCV_FISHEYE", 8),
    CameraModel(6, "FULL_OPENCV", 12), CameraModel(7, "FOV", 5), CameraModel(8, "SIMPLE_RADIAL_FISHEYE", 4),
    CameraModel(9, "RADIAL_FISHEYE", 5), CameraModel(10, "THIN_PRISM_FISHEYE", 12),
]
CAMERA_MODEL_IDS = {m.model_id: m for m in CAMERA_MODELS}
CAMERA_MODEL_NAMES = {m.model_name: m for m in CAMERA_MODELS}

# parameter names per model (colmap2mvsnet.py:305-317); only f / fx / fy / cx / cy are used, distortion is ignored
PARAM_TYPE = {
    "SIMPLE_PINHOLE": ["f", "cx", "cy"],
    "PINHOLE": ["fx", "fy", "cx", "cy"],
    "SIMPLE_RADIAL": ["f", "cx", "cy", "k"],
    "SIMPLE_RADIAL_FISHEYE": ["f", "cx", "cy", "k"],
    "RADIAL": ["f", "cx", "cy", "k1", "k2"],
    "RADIAL_FISHEYE": ["f", "cx", "cy", "k1", "k2"],
    "OPENCV": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"],
    "OPENCV_FISHEYE": ["fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4"],
    "FULL_OPENCV": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"],
    "FOV": ["fx", "fy", "cx", "cy", "omega"],
    "THIN_PRISM_FISHEYE": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "sx1", "sy1"],
}


@dataclass
class Camera:
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray          # float64


@dataclass
class Images:
    """Registered images in file order; observation k of image i is row obs_ptr[i] + k of xys / point3D_ids."""
    ids: np.ndarray             # int64 [N]
    qvecs: np.ndarray           # float64 [N, 4] (w, x, y, z)
    tvecs: np.ndarray           # float64 [N, 3]
    camera_ids: np.ndarray      # int64 [N]
    names: List[str]
    obs_ptr: np.ndarray         # int64 [N + 1]
    xys: np.ndarray             # float64 [M, 2]
    point3D_ids: np.ndarray     # int64 [M]; -1 = no point

    def __len__(self):
        return len(self.names)


@dataclass
class Points3D:
    """Points in file order; the track of point k is rows track_ptr[k]:track_ptr[k + 1] of track_image_ids / track_point2D_idxs."""
    ids: np.ndarray             # int64 [P]
    xyz: np.ndarray             # float64 [P, 3]
    rgb: np.ndarray             # uint8 [P, 3]
    error: np.ndarray           # float64 [P]
    track_ptr: np.ndarray       # int64 [P + 1]
    track_image_ids: np.ndarray     # int32 [T]
    track_point2D_idxs: np.ndarray  # int32 [T]

    def __len__(self):
        return len(self.ids)


@dataclass
class Model:
    cameras: Dict[int, Camera] = field(default_factory=dict)
    images: Images = None
    points3D: Points3D = None


def _ptr(lengths) -> np.ndarray:
    p = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=p[1:])
    return p


def _rows(ptr: np.ndarray) -> np.ndarray:
    """Row-within-record index of every payload element: 0..len-1 per record."""
    n = int(ptr[-1])
    return np.arange(n, dtype=np.int64) - np.repeat(ptr[:-1], np.diff(ptr))


# ---- binary -----------------------------------------------------------------------------------------------------------------
def read_cameras_binary(path: str) -> Dict[int, Camera]:
    data = open(path, "rb").read()
    n = struct.unpack_from("<Q", data, 0)[0]
    off, cams = 8, {}
    for _ in range(n):
        cid, mid, w, h = struct.unpack_from("<iiQQ", data, off)
        off += 24
        if mid not in CAMERA_MODEL_IDS:
            raise ValueError("%s: unknown camera model id %d" % (path, mid))
        m = CAMERA_MODEL_IDS[mid]
        params = np.frombuffer(data, "<f8", m.num_params, off).astype(np.float64)
        off += 8 * m.num_params
        cams[cid] = Camera(cid, m.model_name, w, h, params)
    return cams


def read_images_binary(path: str) -> Images:
    data = open(path, "rb").read()
    n = struct.unpack_from("<Q", data, 0)[0]
    off = 8
    head = np.zeros(n, [("id", "<i8"), ("q", "<f8", 4), ("t", "<f8", 3), ("cam", "<i8")])
    names, starts, counts = [], [], []
    for k in range(n):
        rec = struct.unpack_from("<idddddddi", data, off)
        head[k] = (rec[0], rec[1:5], rec[5:8], rec[8])
        off += 64
        end = data.index(b"\x00", off)
        names.append(data[off:end].decode("utf-8"))
        off = end + 1
        m = struct.unpack_from("<Q", data, off)[0]
        off += 8
        starts.append(off)
        counts.append(m)
        off += 24 * m
    ptr = _ptr(counts)
    buf = np.frombuffer(data, np.uint8)
    # byte offset of every observation record, then the 24-byte records gathered as one structured array
    pos = np.repeat(np.asarray(starts, np.int64), counts) + 24 * _rows(ptr)
    rec = buf[pos[:, None] + np.arange(24)].copy().view([("x", "<f8"), ("y", "<f8"), ("id", "<i8")]).reshape(-1)
    xys = np.stack([rec["x"], rec["y"]], 1).astype(np.float64) if len(rec) else np.zeros((0, 2))
    return Images(head["id"].astype(np.int64), head["q"].astype(np.float64), head["t"].astype(np.float64), head["cam"].astype(np.int64),
                  names, ptr, xys, rec["id"].astype(np.int64))


_POINT_HEAD = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("err", "<f8")])   # 43 bytes, packed


def read_points3D_binary(path: str) -> Points3D:
    data = open(path, "rb").read()
    n = struct.unpack_from("<Q", data, 0)[0]
    unpack = struct.Struct("<Q").unpack_from
    off, offs, lens = 8, [], []
    for _ in range(n):
        L = unpack(data, off + 43)[0]
        offs.append(off)
        lens.append(L)
        off += 51 + 8 * L
    offs = np.asarray(offs, np.int64)
    buf = np.frombuffer(data, np.uint8)
    head = buf[offs[:, None] + np.arange(43)].copy().view(_POINT_HEAD).reshape(-1) if n else np.zeros(0, _POINT_HEAD)
    ptr = _ptr(lens)
    pos = np.repeat(offs + 51, lens) + 8 * _rows(ptr)
    tr = buf[pos[:, None] + np.arange(8)].copy().view([("img", "<i4"), ("p2d", "<i4")]).reshape(-1)
    return Points3D(head["id"].astype(np.int64), head["xyz"].astype(np.float64), head["rgb"].astype(np.uint8), head["err"].astype(np.float64),
                    ptr, tr["img"].astype(np.int32), tr["p2d"].astype(np.int32))


# ---- text -------------------------------------------------------------------------------------------------------------------
def _data_lines(path: str):
    with open(path, "r") as f:
        for line in f:
            s = line.strip()
            if s and s[0] != "#":
                yield s


def read_cameras_text(path: str) -> Dict[int, Camera]:
    cams = {}
    for s in _data_lines(path):
        e = s.split()
        cid = int(e[0])
        if e[1] not in CAMERA_MODEL_NAMES:
            raise ValueError("%s: unknown camera model %r" % (path, e[1]))
        cams[cid] = Camera(cid, e[1], int(e[2]), int(e[3]), np.array([float(x) for x in e[4:]], np.float64))
    return cams


def read_images_text(path: str) -> Images:
    ids, qs, ts, cams, names, counts, xs, ps = [], [], [], [], [], [], [], []
    with open(path, "r") as f:
        while True:
            line = f.readline()
            if not line:
                break
            s = line.strip()
            if not s or s[0] == "#":
                continue
            e = s.split()
            ids.append(int(e[0]))
            qs.append([float(x) for x in e[1:5]])
            ts.append([float(x) for x in e[5:8]])
            cams.append(int(e[8]))
            names.append(e[9])
            obs = f.readline().split()
            xy = np.array(obs[0::3] + obs[1::3], np.float64).reshape(2, -1).T
            xs.append(xy)
            ps.append(np.array(obs[2::3], np.int64))
            counts.append(len(obs) // 3)
    n = len(ids)
    return Images(np.array(ids, np.int64), np.array(qs, np.float64).reshape(n, 4), np.array(ts, np.float64).reshape(n, 3),
                  np.array(cams, np.int64), names, _ptr(counts), np.concatenate(xs) if xs else np.zeros((0, 2)),
                  np.concatenate(ps) if ps else np.zeros(0, np.int64))


def read_points3D_text(path: str) -> Points3D:
    ids, xyz, rgb, err, lens, tracks = [], [], [], [], [], []
    for s in _data_lines(path):
        e = s.split()
        ids.append(int(e[0]))
        xyz.append([float(x) for x in e[1:4]])
        rgb.append([int(x) for x in e[4:7]])
        err.append(float(e[7]))
        tr = np.array(e[8:], np.int64)
        lens.append(len(tr) // 2)
        tracks.append(tr)
    n = len(ids)
    tr = np.concatenate(tracks) if tracks else np.zeros(0, np.int64)
    return Points3D(np.array(ids, np.int64), np.array(xyz, np.float64).reshape(n, 3), np.array(rgb, np.uint8).reshape(n, 3),
                    np.array(err, np.float64), _ptr(lens), tr[0::2].astype(np.int32), tr[1::2].astype(np.int32))


def model_ext(path: str) -> str:
    """'.bin' when the binary model is present in `path`, else '.txt' (the reference reads '.bin' only)."""
    if all(os.path.exists(os.path.join(path, n + ".bin")) for n in ("cameras", "images", "points3D")):
        return ".bin"
    if all(os.path.exists(os.path.join(path, n + ".txt")) for n in ("cameras", "images", "points3D")):
        return ".txt"
    raise FileNotFoundError("no COLMAP model (cameras / images / points3D, .bin or .txt) in %s" % path)


def read_model(path: str, ext: str = None) -> Model:
    ext = ext or model_ext(path)
    if ext == ".bin":
        return Model(read_cameras_binary(os.path.join(path, "cameras.bin")), read_images_binary(os.path.join(path, "images.bin")),
                     read_points3D_binary(os.path.join(path, "points3D.bin")))
    if ext == ".txt":
        return Model(read_cameras_text(os.path.join(path, "cameras.txt")), read_images_text(os.path.join(path, "images.txt")),
                     read_points3D_text(os.path.join(path, "points3D.txt")))
    raise ValueError("model extension must be .bin or .txt, got %r" % ext)


# ---- writers ----------------------------------------------------------------------------------------------------------------
def write_model(model: Model, path: str, ext: str = ".bin") -> None:
    os.makedirs(path, exist_ok=True)
    if ext == ".bin":
        _write_binary(model, path)
    elif ext == ".txt":
        _write_text(model, path)
    else:
        raise ValueError("model extension must be .bin or .txt, got %r" % ext)


def _write_binary(model: Model, path: str) -> None:
    with open(os.path.join(path, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(model.cameras)))
        for c in model.cameras.values():
            m = CAMERA_MODEL_NAMES[c.model]
            f.write(struct.pack("<iiQQ", c.id, m.model_id, c.width, c.height))
            f.write(np.asarray(c.params, "<f8").tobytes())
    im = model.images
    with open(os.path.join(path, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(im)))
        for i in range(len(im)):
            f.write(struct.pack("<idddddddi", int(im.ids[i]), *map(float, im.qvecs[i]), *map(float, im.tvecs[i]), int(im.camera_ids[i])))
            f.write(im.names[i].encode("utf-8") + b"\x00")
            a, b = int(im.obs_ptr[i]), int(im.obs_ptr[i + 1])
            rec = np.zeros(b - a, [("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            rec["x"], rec["y"], rec["id"] = im.xys[a:b, 0], im.xys[a:b, 1], im.point3D_ids[a:b]
            f.write(struct.pack("<Q", b - a))
            f.write(rec.tobytes())
    pt = model.points3D
    with open(os.path.join(path, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(pt)))
        head = np.zeros(len(pt), _POINT_HEAD)
        head["id"], head["xyz"], head["rgb"], head["err"] = pt.ids, pt.xyz, pt.rgb, pt.error
        tr = np.zeros(len(pt.track_image_ids), [("img", "<i4"), ("p2d", "<i4")])
        tr["img"], tr["p2d"] = pt.track_image_ids, pt.track_point2D_idxs
        hb, tb = head.tobytes(), tr.tobytes()
        chunks = []
        for k in range(len(pt)):
            a, b = int(pt.track_ptr[k]), int(pt.track_ptr[k + 1])
            chunks += [hb[43 * k:43 * k + 43], struct.pack("<Q", b - a), tb[8 * a:8 * b]]
        f.write(b"".join(chunks))


def _write_text(model: Model, path: str) -> None:
    r = lambda x: repr(float(x))          # shortest round-trip form: the text model reads back bit for bit
    with open(os.path.join(path, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for c in model.cameras.values():
            f.write(" ".join([str(c.id), c.model, str(c.width), str(c.height)] + [r(p) for p in c.params]) + "\n")
    im = model.images
    with open(os.path.join(path, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for i in range(len(im)):
            f.write(" ".join([str(int(im.ids[i]))] + [r(x) for x in im.qvecs[i]] + [r(x) for x in im.tvecs[i]] +
                             [str(int(im.camera_ids[i])), im.names[i]]) + "\n")
            a, b = int(im.obs_ptr[i]), int(im.obs_ptr[i + 1])
            f.write(" ".join("%s %s %d" % (r(x), r(y), p) for (x, y), p in zip(im.xys[a:b], im.point3D_ids[a:b])) + "\n")
    pt = model.points3D
    with open(os.path.join(path, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for k in range(len(pt)):
            a, b = int(pt.track_ptr[k]), int(pt.track_ptr[k + 1])
            tr = " ".join("%d %d" % (i, j) for i, j in zip(pt.track_image_ids[a:b], pt.track_point2D_idxs[a:b]))
            f.write(" ".join([str(int(pt.ids[k]))] + [r(x) for x in pt.xyz[k]] + [str(int(x)) for x in pt.rgb[k]] + [r(pt.error[k])]) +
                    (" " + tr if tr else "") + "\n")


# ---- camera matrices --------------------------------------------------------------------------------------------------------
def intrinsic(cam: Camera) -> np.ndarray:
    """K as colmap2mvsnet.py:319-331 builds it: `f` sets fx and fy, distortion parameters are ignored."""
    if cam.model not in PARAM_TYPE:
        raise ValueError("unknown camera model %r" % cam.model)
    d = {k: v for k, v in zip(PARAM_TYPE[cam.model], cam.params)}
    if "f" in PARAM_TYPE[cam.model]:
        d["fx"] = d["f"]
        d["fy"] = d["f"]
    return np.array([[d["fx"], 0, d["cx"]], [0, d["fy"], d["cy"]], [0, 0, 1]], np.float64)


def qvec2rotmat(q: np.ndarray) -> np.ndarray:
    """[..., 4] -> [..., 3, 3] in fp64, element expressions in colmap2mvsnet.py:250-261's order (the same bits per element)."""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    # the reference squares numpy scalars, which is libm's pow(v, 2.0); numpy's array square is v * v and differs in the last
    # bit for about 0.1 % of the values, so the squares go through Python's float pow element by element
    sq = np.array([v ** 2 for v in q.ravel().tolist()], np.float64).reshape(q.shape)
    x2, y2, z2 = sq[..., 1], sq[..., 2], sq[..., 3]
    R = np.stack([
        1 - 2 * y2 - 2 * z2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y,
        2 * x * y + 2 * w * z, 1 - 2 * x2 - 2 * z2, 2 * y * z - 2 * w * x,
        2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x2 - 2 * y2], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def extrinsics(images: Images) -> np.ndarray:
    """[N, 4, 4] fp64 world-to-camera matrices [R t; 0 1] (colmap2mvsnet.py:334-341)."""
    n = len(images)
    E = np.zeros((n, 4, 4), np.float64)
    E[:, :3, :3] = qvec2rotmat(images.qvecs)
    E[:, :3, 3] = images.tvecs
    E[:, 3, 3] = 1
    return E


def camera_centres(E: np.ndarray) -> np.ndarray:
    """C = -R^T t per image, [N, 3] fp64; each component summed left to right without fused multiply-adds."""
    R, t = E[:, :3, :3], E[:, :3, 3]
    return -(R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2] + R[:, 2, :] * t[:, 2:3])
