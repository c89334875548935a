"""The on-disk formats between inference and depth-map filtering, written and read byte-compatibly
with the reference so that either side can be swapped on its own:

    depth      ``depth_est/<view>.pfm``      greyscale PFM, float32, bottom row first, negative scale = little endian
                                             (datasets/data_io.py:7-37 read_pfm, :40-67 save_pfm)
    confidence ``confidence/<view>.npy``     uint8 = floor(photometric_confidence * 255)          (test.py:281-286)
    camera     ``cams/<view>_cam.txt``       "extrinsic" 4x4, blank line, "intrinsic" 3x3, blank line, the 4 values of the
                                             intrinsic slot's last row (depth range)             (test.py:149-166, :102-112)
    image      ``images/<view>.jpg``         RGB, decoded with PIL                               (test.py:116-121)
    pairs      ``pair.txt`` / ``new_pair.txt``  view count, then per view its id and "n id score id score ..."
                                             (test.py:136-146, test_tt.py:142-156)
    point cloud ``<scan>.ply``               binary little-endian PLY, vertex {float x, y, z; uchar red, green, blue}
                                             (test.py:431-442, written there with plyfile)
    Gipuma     ``points_mvsnet/``            fusibile's input folder: cams/<image>.P, images/, 2333__<view>/disp.dmb and
                                             normals.dmb (misc/gipuma.py:25-157)

Host-side numpy only; nothing here touches the GPU.
"""
from __future__ import annotations

import os
import re
import shutil
import struct
import sys
from typing import List, Tuple

import numpy as np


def read_pfm(filename: str) -> Tuple[np.ndarray, float]:
    """-> (image [H,W] or [H,W,3] float32 with the TOP row first, scale)."""
    with open(filename, "rb") as f:
        header = f.readline().decode("utf-8").rstrip()
        if header not in ("PF", "Pf"):
            raise Exception("Not a PFM file.")
        color = header == "PF"
        m = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if not m:
            raise Exception("Malformed PFM header.")
        width, height = int(m.group(1)), int(m.group(2))
        scale = float(f.readline().rstrip())
        endian = "<" if scale < 0 else ">"
        data = np.fromfile(f, endian + "f")
    shape = (height, width, 3) if color else (height, width)
    return np.flipud(np.reshape(data, shape)), abs(scale)


def save_pfm(filename: str, image: np.ndarray, scale: float = 1) -> None:
    if image.dtype.name != "float32":
        raise Exception("Image dtype must be float32.")
    if image.ndim == 3 and image.shape[2] == 3:
        color = True
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        color = False
    else:
        raise Exception("Image must have H x W x 3, H x W x 1 or H x W dimensions.")
    image = np.flipud(image)
    little = image.dtype.byteorder == "<" or (image.dtype.byteorder == "=" and sys.byteorder == "little")
    with open(filename, "wb") as f:
        f.write(b"PF\n" if color else b"Pf\n")
        f.write(("%d %d\n" % (image.shape[1], image.shape[0])).encode("utf-8"))
        f.write(("%f\n" % (-scale if little else scale)).encode("utf-8"))
        image.tofile(f)


def save_confidence(filename: str, photometric_confidence: np.ndarray) -> None:
    np.save(filename, (photometric_confidence * 255).astype(np.uint8))


def load_confidence(filename: str) -> np.ndarray:
    return np.load(filename)


def write_cam(filename: str, cam: np.ndarray) -> None:
    """cam [2,4,4]: 0 = extrinsic, 1 = intrinsic in the top-left 3x3 with the depth range in its last row."""
    with open(filename, "w") as f:
        f.write("extrinsic\n")
        for i in range(4):
            f.write("".join(str(cam[0][i][j]) + " " for j in range(4)) + "\n")
        f.write("\nintrinsic\n")
        for i in range(3):
            f.write("".join(str(cam[1][i][j]) + " " for j in range(3)) + "\n")
        f.write("\n" + " ".join(str(cam[1][3][j]) for j in range(4)) + "\n")


def read_camera_parameters(filename: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (intrinsics [3,3], extrinsics [4,4]) float32."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intrinsics, extrinsics


def read_img(filename: str) -> np.ndarray:
    """-> [H,W,3] uint8, the decoded RGB bytes.  The reference (test.py:116-121) scales them to float32 / 255 and its drivers
    multiply the kept colours by 255 again before the uint8 cast (:421-424); that round trip is the identity on all 256 values,
    so the bytes are kept as they are."""
    from PIL import Image
    with Image.open(filename) as img:
        if img.mode != "RGB":
            img = img.convert("RGB")
        return np.array(img, dtype=np.uint8)


def read_pair_file(filename: str, convention: str = "dtu", nviews: int = 10) -> List[Tuple[int, List[int]]]:
    """-> [(ref_view, [src_view, ...]), ...] in file order.  Lines with no source view are dropped (test.py:144).
    convention "dtu" (test.py:136-146): the sources as listed (the dataset later keeps the first 10, test.py:337).
    convention "tt" (test_tt.py:142-156): a list shorter than `nviews` (--fusion_view) is padded with its first source up to
    `nviews`, then `nviews - 1` sources are kept."""
    if convention not in ("dtu", "tt"):
        raise ValueError("read_pair_file: convention must be 'dtu' or 'tt', not %r" % (convention,))
    data = []
    with open(filename) as f:
        num_viewpoint = int(f.readline())
        for _ in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if len(src_views) == 0:
                continue
            if convention == "tt":
                if len(src_views) < nviews:
                    src_views += [src_views[0]] * (nviews - len(src_views))
                src_views = src_views[:nviews - 1]
            data.append((ref_view, src_views))
    return data


# the vertex layout of the reference's PLY (test.py:431-439): plyfile describes a structured array with these fields
PLY_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
              "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
              "double": "<f8", "float64": "<f8"}


def ply_header(n: int) -> bytes:
    """The header plyfile writes for the reference's vertex array (PlyElement.describe(vertex_all, 'vertex'), test.py:440-441).
    The type names `float` / `uchar` are plyfile's names for numpy 'f4' / 'u1' (its type table); they have not been compared
    with a file plyfile itself wrote."""
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n] + \
        ["property float %s" % c for c in "xyz"] + ["property uchar %s" % c for c in ("red", "green", "blue")] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def write_ply_records(filename: str, records) -> None:
    """records: the packed PLY body, 15 bytes per vertex in PLY_VERTEX_DTYPE layout (bytes-like or uint8 / structured array)."""
    body = memoryview(np.ascontiguousarray(records)).cast("B")
    if body.nbytes % PLY_VERTEX_DTYPE.itemsize:
        raise ValueError("write_ply_records: %d bytes is not a whole number of %d-byte vertices" % (body.nbytes, PLY_VERTEX_DTYPE.itemsize))
    with open(filename, "wb") as f:
        f.write(ply_header(body.nbytes // PLY_VERTEX_DTYPE.itemsize))
        f.write(body)


def write_ply(filename: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """xyz [N,3] float32, rgb [N,3] uint8 -> binary little-endian PLY, the file test.py:431-442 writes with plyfile."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError("write_ply: want xyz [N,3] and rgb [N,3], got %s and %s" % (xyz.shape, rgb.shape))
    v = np.empty(xyz.shape[0], PLY_VERTEX_DTYPE)
    for i, c in enumerate("xyz"):
        v[c] = xyz[:, i]
    for i, c in enumerate(("red", "green", "blue")):
        v[c] = rgb[:, i]
    write_ply_records(filename, v)


def read_ply(filename: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (xyz [N,3] float32, rgb [N,3] uint8) of a binary little-endian PLY whose only element is `vertex` with (at least)
    x, y, z and red, green, blue properties of fixed size."""
    with open(filename, "rb") as f:
        if f.readline().rstrip(b"\r\n") != b"ply":
            raise ValueError("%s: not a PLY file" % filename)
        n, fields, elements = None, [], []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header without end_header" % filename)
            tok = line.decode("ascii").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "end_header":
                break
            if tok[0] == "format":
                if tok[1] != "binary_little_endian":
                    raise ValueError("%s: PLY format %s is not supported (binary_little_endian only)" % (filename, tok[1]))
            elif tok[0] == "element":
                elements.append(tok[1])
                if tok[1] == "vertex":
                    n = int(tok[2])
            elif tok[0] == "property":
                if tok[1] == "list" or tok[1] not in _PLY_TYPES:
                    raise ValueError("%s: PLY property %r is not supported" % (filename, " ".join(tok[1:])))
                if elements[-1:] == ["vertex"]:
                    fields.append((tok[2], _PLY_TYPES[tok[1]]))
        if elements != ["vertex"] or n is None:
            raise ValueError("%s: want exactly one PLY element, vertex (got %s)" % (filename, elements))
        v = np.frombuffer(f.read(), dtype=np.dtype(fields), count=n)
    xyz = np.stack([v[c] for c in "xyz"], -1).astype(np.float32)
    rgb = np.stack([v[c] for c in ("red", "green", "blue")], -1).astype(np.uint8)
    return xyz, rgb


# ---------------------------------------------------------------- Gipuma / fusibile formats (misc/gipuma.py:25-157)
def read_gipuma_dmb(path: str) -> np.ndarray:
    """A Gipuma .dmb image: int32 type, height, width, channels, then the float32 samples, channel-planar -> [H,W] or [H,W,C]
    (misc/gipuma.py:25-36)."""
    with open(path, "rb") as f:
        _, height, width, channels = struct.unpack("<4i", f.read(16))
        data = np.fromfile(f, np.float32)
    return np.transpose(data.reshape((width, height, channels), order="F"), (1, 0, 2)).squeeze()


def write_gipuma_dmb(path: str, image: np.ndarray) -> None:
    """[H,W] or [H,W,C] -> .dmb (misc/gipuma.py:39-60): the samples are written in the array's own dtype, [C,H,W] order."""
    image = np.asarray(image)
    height, width = image.shape[0], image.shape[1]
    channels = image.shape[2] if image.ndim == 3 else 1
    if image.ndim == 3:
        image = np.transpose(image, (2, 0, 1)).squeeze()
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", 1, height, width, channels))
        image.tofile(f)


def gipuma_projection(intrinsics: np.ndarray, extrinsics: np.ndarray) -> np.ndarray:
    """P = [K 0; 0 0] E, first three rows, in float64 from the float32 file values (misc/gipuma.py:72-80) -> [3,4]."""
    k4 = np.zeros((4, 4))
    k4[:3, :3] = intrinsics
    return np.matmul(k4, extrinsics)[0:3]


def write_gipuma_cam(path: str, intrinsics: np.ndarray, extrinsics: np.ndarray) -> None:
    """The .P file fusibile reads: P's 12 float64 values as str() writes them, each followed by a space, one row per line, then
    an empty line (misc/gipuma.py:82-90)."""
    P = gipuma_projection(intrinsics, extrinsics)
    with open(path, "w") as f:
        for i in range(3):
            f.write("".join(str(P[i][j]) + " " for j in range(4)) + "\n")
        f.write("\n")


def gipuma_view_names(scan_folder: str) -> List[str]:
    """The image file names of a scene (images/, hidden files skipped), sorted: the Gipuma route's view set and order."""
    folder = os.path.join(scan_folder, "images")
    if not os.path.isdir(folder):
        raise ValueError("%s: no images/ folder" % scan_folder)
    return sorted(n for n in os.listdir(folder) if not n.startswith("."))


def gipuma_prob_filter(depth: np.ndarray, prob: np.ndarray, prob_threshold: float) -> np.ndarray:
    """misc/gipuma.py:172-179: a uint8 map is divided by 255 (float64), any other is compared in its own dtype; depth is kept
    where prob > prob_threshold and set to 0 elsewhere (a filtered copy is returned)."""
    if prob.dtype == np.uint8:
        prob = prob / 255
    out = np.array(depth, copy=True)
    out[~(prob > prob_threshold)] = 0
    return out


def export_gipuma_folder(scan_folder: str, point_folder: str, prob_threshold: float = 0.5, write_filtered: bool = False) -> List[str]:
    """The probability filter and the conversion of misc/gipuma.py:116-181 (probability_filter + mvsnet_to_gipuma): write
    fusibile's input folder `point_folder` (cams/<image>.P, images/ copied, 2333__<view>/disp.dmb and normals.dmb with the
    reference's fake normals).  depth_est/<view>_prob_filtered.pfm is written next to the depth maps only with write_filtered.
    -> the view names (sorted image names).  Running fusibile on the folder is left to the caller."""
    names = gipuma_view_names(scan_folder)
    for sub in ("", "cams", "images"):
        os.makedirs(os.path.join(point_folder, sub), exist_ok=True)
    for name in names:
        prefix = os.path.splitext(name)[0]
        K, E = read_camera_parameters(os.path.join(scan_folder, "cams", prefix + "_cam.txt"))
        write_gipuma_cam(os.path.join(point_folder, "cams", name + ".P"), K, E)
        shutil.copy(os.path.join(scan_folder, "images", name), os.path.join(point_folder, "images", name))
        depth, _ = read_pfm(os.path.join(scan_folder, "depth_est", prefix + ".pfm"))
        depth = gipuma_prob_filter(depth, np.load(os.path.join(scan_folder, "confidence", prefix + ".npy")), prob_threshold)
        if write_filtered:
            save_pfm(os.path.join(scan_folder, "depth_est", prefix + "_prob_filtered.pfm"), depth)
        sub = os.path.join(point_folder, "2333__" + prefix)
        os.makedirs(sub, exist_ok=True)
        write_gipuma_dmb(os.path.join(sub, "disp.dmb"), depth)
        # fake normals (misc/gipuma.py:95-113): (1, 1, 1) / 1.732050808 where the depth read back from disp.dmb is > 0
        d = read_gipuma_dmb(os.path.join(sub, "disp.dmb"))
        mask = np.tile(np.where(d > 0, 1, 0).reshape(d.shape[0], d.shape[1], 1), [1, 1, 3]).astype(np.float32)
        normal = np.tile(np.ones_like(d).reshape(d.shape[0], d.shape[1], 1), [1, 1, 3]) / 1.732050808
        write_gipuma_dmb(os.path.join(sub, "normals.dmb"), np.float32(np.multiply(normal, mask)))
    return names
