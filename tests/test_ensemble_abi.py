"""CPU-side checks of aoc_track_ensemble: every argument error is reported with its reason before anything touches a
device, the ABI revision and the struct sizes are what they were, batch.track_ensemble's packing of `nominal` and its
dealing of members to optima work on NumPy inputs, and the host loop the GPU tests compare with reproduces the
reference's closed-loop run."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from aircraftoptimalcontrol_amd import _lib


def _prob(B=64, T=10):
    p = _lib.Problem()
    p.B, p.T = B, T
    p.RRt[:] = [1e-5, 0.0, 0.0, 1e-5]
    return p


def test_argument_errors_carry_a_reason():
    _lib.build_library()
    lib = _lib.lib()
    call = lambda p, n_opt=1, mpo=64, nominal=1, x0=1, noise=None, x=None, u=None, dist=None, stats=1, status=None: \
        lib.aoc_track_ensemble(C.byref(p) if p is not None else None, n_opt, mpo, nominal, x0, noise, x, u, dist, stats, status)
    nz = C.byref(_lib.MpcNoise(1, 0, 0, (C.c_double * 6)(*[1e-3] * 6)))
    f32 = _prob()
    f32.x_out_f32 = 1
    rsym = _prob()
    rsym.RRt[1] = 1e-7
    cases = [
        (dict(p=None), b"aoc_problem is NULL"),
        (dict(p=_prob(), nominal=None), b"nominal is NULL"),
        (dict(p=_prob(), x0=None), b"x0_reg is NULL"),
        (dict(p=_prob(), stats=None), b"stats is NULL"),
        (dict(p=_prob(), n_opt=0), b"n_opt = 0"),
        (dict(p=_prob(), mpo=0), b"members_per_opt = 0"),
        (dict(p=_prob(), mpo=100), b"members_per_opt = 100"),
        (dict(p=_prob(), mpo=-64), b"members_per_opt = -64"),
        (dict(p=_prob(T=2)), b"T = 2"),
        (dict(p=_prob(B=65)), b"B = 65"),                          # more members than n_opt * members_per_opt
        (dict(p=_prob(B=128), n_opt=3), b"B = 128"),               # the last group would be empty
        (dict(p=_prob(B=0)), b"B = 0"),
        (dict(p=_prob(), x=1), b"x_reg and u_reg go together"),
        (dict(p=_prob(), u=1), b"x_reg and u_reg go together"),
        (dict(p=f32, x=1, u=1, noise=nz), b"float32"),
        (dict(p=rsym), b"RRt is not symmetric"),
    ]
    for kw, reason in cases:
        # leave another reason behind first, so that an error return without a new reason shows
        q = _lib.Problem()
        q.B, q.T, q.ref = 4, 2, 1
        assert lib.aoc_traj_cost(C.byref(q), 1, 1, 1, 1) == -1 and b"T = 2 " in lib.aoc_last_hip_error() + b" "
        assert call(**kw) == -1, kw
        msg = lib.aoc_last_hip_error()
        assert b"aoc_track_ensemble" in msg and reason in msg, (kw, msg)


def test_abi_revision_and_struct_sizes_unchanged():
    lib = _lib.lib()
    assert lib.aoc_abi_version() == _lib.AOC_ABI_VERSION == 5
    assert C.sizeof(_lib.Model) == 72
    assert C.sizeof(_lib.Problem) == 72 + 76 * 8 + 32 + 16
    assert C.sizeof(_lib.Params) == 48
    assert C.sizeof(_lib.Tuning) == 104
    assert C.sizeof(_lib.MpcNoise) == 64
    assert "aoc_track_ensemble" in _lib.SYMBOLS and _lib.AOC_ENS_NSTAT == 16


def test_nominal_packing_and_group_mapping():
    from aircraftoptimalcontrol_amd import batch
    rng = np.random.default_rng(0)
    n, T = 3, 7
    xo, uo, KK = rng.normal(size=(n, 6, T)), rng.normal(size=(n, 2, T)), rng.normal(size=(n, 2, 6, T))
    nom = batch.ensemble_nominal(xo, uo, KK)
    assert nom.shape == (n, T, 20) and nom.flags.c_contiguous and nom.dtype == np.float64
    for k in range(n):
        for t in range(T):
            rec = nom[k, t]
            assert np.array_equal(rec[0:6], xo[k, :, t]) and np.array_equal(rec[6:8], uo[k, :, t])
            assert np.array_equal(rec[8:14], KK[k, 0, :, t]) and np.array_equal(rec[14:20], KK[k, 1, :, t])
    with pytest.raises(ValueError):
        batch.ensemble_nominal(xo, uo, KK[:, :, :, :-1])
    # members are dealt by whole tiles; the last group may be partial, none empty
    mpo, grp = batch.ensemble_groups(322, 2, 192)
    assert mpo == 192 and np.array_equal(grp, np.r_[np.zeros(192, int), np.ones(130, int)])
    assert batch.ensemble_groups(65536, 1)[0] == 65536
    assert batch.ensemble_groups(100, 1)[0] == 128
    mpo, grp = batch.ensemble_groups(1000, 3)                     # ceil(1000 / 3) = 334 -> 384 per optimum
    assert mpo == 384 and np.array_equal(np.bincount(grp), [384, 384, 232])
    for bad in ((322, 2, 100), (322, 2, 128), (322, 3, 192), (64, 1, 0), (0, 1, 64), (128, 3, None)):
        with pytest.raises(ValueError):
            batch.ensemble_groups(*bad)


def test_host_loop_reproduces_the_reference_run():
    """The checker of tests/test_gpu_ensemble.py on its own: with the reference's gains and delta = 0.1 the host loop
    gives the reference's xx_reg and uu_reg bit for bit, and its cost restatement the oracle's traj_cost to rounding."""
    from oracle import oracle as orc
    from test_gpu_ensemble import host_cost, host_loop, numpy_stats
    g = load_golden("g4_lqr_tracking")
    mdl = orc.default_model(float(g["dt"]))
    T = g["xx_opt"].shape[1]
    xx, uu = host_loop(mdl, g["xx_opt"], g["uu_opt"], g["KK"], (g["xx_opt"][:, 0] + 0.1)[None])
    assert np.array_equal(xx[0], g["xx_reg"]) and np.array_equal(uu[0], g["uu_reg"])
    J = host_cost(g["QQt"], g["RRt"], g["QQT"], xx, uu, g["xx_opt"], g["uu_opt"])
    op = orc.OracleProblem(g["QQt"], g["RRt"], g["QQT"], g["xx_opt"], g["uu_opt"], float(g["dt"]))
    assert abs(J[0] - orc.traj_cost(op, xx[0], uu[0])) <= 1e-12 * abs(J[0])
    s = numpy_stats(xx, uu, g["xx_opt"], g["uu_opt"], J)
    assert s[0, 15] == T and np.array_equal(s[0, 9:15], xx[0, :, -1] - g["xx_opt"][:, -1])
    assert np.array_equal(s[0, 0:6], np.abs(xx[0] - g["xx_opt"]).max(axis=1))
