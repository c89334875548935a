"""GPU (MI355X): colmap2mvsnet on the device - fixture F24, the CPU file's oracle models and edge cases, a large model (1 000
images, 1 M points, heavy-tailed tracks up to 60 long) against the fp64 oracle, and run-to-run bit identity of the score matrix
and of pair.txt."""
import os

import numpy as np
import pytest
import torch

import colmap_ref as R
import test_colmap as T
from mvsformerplusplus_amd import colmap, colmap2mvsnet as CM, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", T.F24_CASES)
def test_f24_gpu(tmp_path, case):
    T.check_f24_case(DEV, case, str(tmp_path))


@pytest.mark.parametrize("n,p,seed,kw", T.ORACLE_MODELS)
def test_scores_and_depths_vs_oracle_gpu(n, p, seed, kw):
    T.check_oracle_model(DEV, n, p, seed, kw)


def test_edge_cases_gpu():
    T.check_deviation_clamp(DEV)
    T.check_tie_rule_small(DEV)


def test_large_model_vs_oracle_gpu():
    m = synth.make_colmap_model(1000, 1000000, seed=3, tail=2.0, max_track=60, duplicates=0.01, invalid=0.01)
    assert np.diff(m.points3D.track_ptr).max() >= 55
    E = colmap.extrinsics(m.images)
    obs = CM.Observations(m, DEV)
    xyz = torch.from_numpy(m.points3D.xyz).to(DEV)
    S = CM.score_matrix(obs, xyz, E).cpu().numpy()
    So = R.scores(m)
    assert np.array_equal(S == 0, So == 0) and np.array_equal(S, S.T)
    nz = So != 0
    assert np.all(np.abs(S[nz] - So[nz]) <= 1e-12 * So[nz])
    lo, hi = CM.depth_bounds(obs, xyz, E)
    rlo, rhi = R.depth_bounds(m)
    assert np.all(np.abs(lo - rlo) <= 1e-12 * np.abs(rlo)) and np.all(np.abs(hi - rhi) <= 1e-12 * np.abs(rhi))


def test_bitwise_reproducible_gpu(tmp_path):
    m = synth.make_colmap_model(400, 300000, seed=8, tail=1.5, max_track=60, duplicates=0.02, invalid=0.02)
    E = colmap.extrinsics(m.images)
    obs = CM.Observations(m, DEV)
    xyz = torch.from_numpy(m.points3D.xyz).to(DEV)
    a = CM.score_matrix(obs, xyz, E).cpu().numpy()
    b = CM.score_matrix(obs, xyz, E).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    colmap.write_model(m, str(tmp_path / "sparse"), ".bin")
    os.makedirs(str(tmp_path / "images_col"))
    for name in m.images.names:
        with open(str(tmp_path / "images_col" / name), "wb") as f:
            f.write(name.encode())
    CM.convert(str(tmp_path), device=DEV)
    first = open(str(tmp_path / "pair.txt"), "rb").read()
    CM.convert(str(tmp_path), device=DEV)
    assert open(str(tmp_path / "pair.txt"), "rb").read() == first
