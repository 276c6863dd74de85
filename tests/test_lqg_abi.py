"""CPU-side checks of aoc_track_ensemble_lqg: the ABI revision is what it was, the new symbols are declared, exported and
bound, every argument error is reported with its reason before anything touches a device, the scratch query; the fourth-word-1
stream of the host's restatement of the generator; batch.filter_gains; and the host checker of tests/test_gpu_lqg.py — with
zero gains, against the filter's own covariance in a Monte Carlo of the oracle's closed loop, and its own rounding (REF_GAP)."""
import ctypes as C

import numpy as np
import pytest

from aircraftoptimalcontrol_amd import _lib

REC = 56 * 8   # bytes of scratch per (optimum, sample)


def _prob(T=10, B=64):
    p = _lib.Problem()
    p.B, p.T = B, T
    return p


def test_abi_revision_and_symbols():
    _lib.build_library()
    lib = _lib.lib()
    assert lib.aoc_abi_version() == _lib.AOC_ABI_VERSION == 5
    assert C.sizeof(_lib.Problem) == 72 + 76 * 8 + 32 + 16 and C.sizeof(_lib.MpcNoise) == 64
    assert _lib.AOC_LQG_NSTAT == 12 and _lib.AOC_ENS_NSTAT == 16
    for name in ("aoc_track_ensemble_lqg", "aoc_track_ensemble_lqg_scratch_bytes"):
        assert name in _lib.SYMBOLS and getattr(lib, name)
    hdr = open(_lib._HDR).read()
    assert "#define AOC_LQG_NSTAT 12" in hdr and "#define AOC_ABI_VERSION 5" in hdr
    assert "size_t aoc_track_ensemble_lqg_scratch_bytes(int32_t n_opt, int32_t T);" in hdr
    assert "still 5, an addition: aoc_track_ensemble_lqg" in hdr
    assert len(_lib.SYMBOLS["aoc_track_ensemble_lqg"][1]) == 19
    # the entry points before it keep their argument lists
    assert len(_lib.SYMBOLS["aoc_track_ensemble"][1]) == 11
    assert len(_lib.SYMBOLS["aoc_track_ensemble_envelope"][1]) == 14
    assert len(_lib.SYMBOLS["aoc_track_ensemble_histogram"][1]) == 15
    assert len(_lib.SYMBOLS["aoc_track_covariance"][1]) == 10


def test_scratch_query():
    """the records of the covariance call's first kernel: one per optimum and sample; a refused geometry asks for nothing"""
    q = _lib.lib().aoc_track_ensemble_lqg_scratch_bytes
    assert q(1, 3) == 3 * REC
    assert q(1, 1000) == 1000 * REC and q(70, 33) == 70 * 33 * REC
    assert q(1 << 20, 1 << 20) == (1 << 40) * REC          # no 32-bit product on the way
    assert q(0, 10) == 0 and q(-1, 10) == 0 and q(1, 2) == 0 and q(1, 0) == 0 and q(1, -5) == 0
    assert q(3, 17) == _lib.lib().aoc_track_covariance_scratch_bytes(3, 17)


def test_argument_errors_carry_a_reason():
    lib = _lib.lib()
    big = 1 << 40
    six = lambda *v: (C.c_double * 6)(*v)
    nz = _lib.MpcNoise(1, 0, 0, six(0, 0, 0, 0, 0, 0))

    def call(p, n_opt=1, mpo=64, nominal=16, filter=16, x0_reg=16, ehat0=None, noise=None, rho=None, x_reg=None, u_reg=None,
             xhat=None, dist=None, meas=None, stats=16, est_stats=16, status=None, scratch=16, scratch_bytes=big):
        return lib.aoc_track_ensemble_lqg(C.byref(p) if p is not None else None, n_opt, mpo, nominal, filter, x0_reg, ehat0,
                                          C.byref(noise) if noise is not None else None, rho, x_reg, u_reg, xhat, dist, meas,
                                          stats, est_stats, status, scratch, scratch_bytes)
    need = lib.aoc_track_ensemble_lqg_scratch_bytes(2, 10)
    assert need == 2 * 10 * REC
    f32 = _prob()
    f32.x_out_f32 = 1
    skew = _prob()
    skew.RRt[1], skew.RRt[2] = 1.0, 2.0
    cases = [
        # the refusals of aoc_track_ensemble
        (dict(p=None), b"aoc_problem is NULL"),
        (dict(p=_prob(), nominal=None), b"nominal is NULL"),
        (dict(p=_prob(), x0_reg=None), b"x0_reg is NULL"),
        (dict(p=_prob(), stats=None), b"stats is NULL"),
        (dict(p=_prob(), n_opt=0), b"n_opt = 0"),
        (dict(p=_prob(), mpo=32), b"members_per_opt = 32"),
        (dict(p=_prob(), mpo=96), b"members_per_opt = 96"),
        (dict(p=_prob(B=65)), b"B = 65 members do not fill"),
        (dict(p=_prob(B=64), n_opt=2), b"B = 64 members do not fill"),
        (dict(p=_prob(), x_reg=16), b"x_reg and u_reg go together"),
        (dict(p=_prob(), u_reg=16), b"x_reg and u_reg go together"),
        (dict(p=f32, x_reg=16, u_reg=16, noise=nz), b"float32"),
        (dict(p=skew), b"RRt is not symmetric"),
        # its own
        (dict(p=_prob(), filter=None), b"filter is NULL"),
        (dict(p=_prob(), est_stats=None), b"est_stats is NULL"),
        (dict(p=_prob(T=2)), b"T = 2"),
        (dict(p=_prob(T=0)), b"T = 0"),
        (dict(p=_prob(), rho=six(1, 1, 1, 1, 1, 1)), b"rho without noise"),
        (dict(p=_prob(), rho=six(0, 0, 0, 0, 0, 0)), b"rho without noise"),
        (dict(p=_prob(), noise=nz, rho=six(1, 1, -1e-300, 1, 1, 1)), b"rho[2]"),
        (dict(p=_prob(), noise=nz, rho=six(1, 1, 1, 1, 1, float("nan"))), b"rho[5]"),
        (dict(p=_prob(), noise=nz, rho=six(float("inf"), 1, 1, 1, 1, 1)), b"rho[0]"),
        (dict(p=_prob(), scratch=None), b"scratch is NULL"),
        (dict(p=_prob(), scratch=24), b"16-byte aligned"),
        (dict(p=_prob(B=128), n_opt=2, scratch_bytes=need - 1), b"scratch_bytes = %d, need %d" % (need - 1, need)),
        (dict(p=_prob(), scratch_bytes=0), b"scratch_bytes = 0"),
    ]
    for kw, reason in cases:
        # leave another reason behind first, so that an error return without a new reason shows
        q = _lib.Problem()
        q.B, q.T, q.ref = 4, 2, 1
        assert lib.aoc_traj_cost(C.byref(q), 1, 1, 1, 1) == -1 and b"T = 2 " in lib.aoc_last_hip_error() + b" "
        assert call(**kw) == -1, kw
        msg = lib.aoc_last_hip_error()
        assert msg.startswith(b"aoc_track_ensemble_lqg: ") and reason in msg, (kw, msg)
    # and a neighbour still names itself
    assert lib.aoc_track_ensemble(C.byref(_prob()), 1, 64, None, 1, None, None, None, None, 1, None) == -1
    assert lib.aoc_last_hip_error().startswith(b"aoc_track_ensemble: ")


def test_track_ensemble_refuses_what_does_not_combine():
    """the keyword checks of batch.track_ensemble come before anything touches a device"""
    from aircraftoptimalcontrol_amd import batch

    class P:
        device, T = "cpu", 5
    xo, uo, L = np.zeros((6, 5)), np.zeros((2, 5)), np.zeros((6, 6, 5))
    for kw in (dict(envelope=True), dict(quantiles=(0.5,)), dict(predict=True)):
        with pytest.raises(ValueError, match="does not combine"):
            batch.track_ensemble(P(), xo, uo, delta=np.zeros((4, 6)), filter=L, **kw)
    for kw in (dict(rho=np.ones(6)), dict(ehat0=np.zeros(6))):
        with pytest.raises(ValueError, match="go with filter="):
            batch.track_ensemble(P(), xo, uo, delta=np.zeros((4, 6)), **kw)


def test_measurement_stream_of_the_host_restatement():
    """mpc.noise_draws(..., word3=1) against a known answer computed from mpc.philox4x32_10 with the counter (member, step,
    pair, 1), written out here once more; it differs from the disturbance's stream, which the default still gives."""
    from aircraftoptimalcontrol_amd import mpc
    seed, step, first, B = (0x1234 << 32) | 0xCAFE, 9, 5, 7
    rho = np.array([0.5, 1.0, 2.0, 3.0, 4.0, 5.0])
    got = mpc.noise_draws(seed, step, first, B, rho, 1)
    want = np.zeros((B, 6))
    for b in range(B):
        for j in range(3):
            w = [int(v[0]) for v in mpc.philox4x32_10([first + b], [step], [j], [1], [0xCAFE], [0x1234])]
            u1 = ((w[0] >> 5) * 67108864.0 + (w[1] >> 6) + 1.0) * 2.0 ** -53
            u2 = ((w[2] >> 5) * 67108864.0 + (w[3] >> 6) + 1.0) * 2.0 ** -53
            rad = np.sqrt(-2.0 * np.log(u1))
            want[b, 2 * j] = rho[2 * j] * (rad * np.cos(6.283185307179586476925 * u2))
            want[b, 2 * j + 1] = rho[2 * j + 1] * (rad * np.sin(6.283185307179586476925 * u2))
    assert np.array_equal(got, want)
    word0 = mpc.noise_draws(seed, step, first, B, rho)
    assert np.array_equal(word0, mpc.noise_draws(seed, step, first, B, rho, 0))
    assert (got != word0).all()
    assert abs(got / rho).max() < 6 and abs(got / rho).std() > 0.3


def test_filter_gains_is_the_kalman_recursion():
    """L (P^- + V) = P^-, P^+ = (I - L) P^- (the Joseph form's value), P^-' = A P^+ A^T + W; the filter filters: P^+ < P^- and
    P^+ < V on the diagonal; rho must be positive."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_covariance import g4_jacobians
    from test_gpu_lqg import RHO
    from test_gpu_ensemble import DELTA_SCALE, SIGMA
    g, _, (A, B, _) = g4_jacobians()
    T = 40
    xo, uo = g["xx_opt"][:, :T], g["uu_opt"][:, :T]
    S0 = np.diag((0.1 * DELTA_SCALE) ** 2)
    L, Pm, Pp = batch.filter_gains(None, xo, uo, S0, SIGMA, RHO, jac=(A[:T - 1], B[:T - 1]))
    assert L.shape == Pm.shape == Pp.shape == (6, 6, T) and np.array_equal(Pm[:, :, 0], S0)
    V, W = np.diag(RHO ** 2), np.diag(SIGMA ** 2)
    for t in range(T):
        assert np.allclose(L[:, :, t] @ (Pm[:, :, t] + V), Pm[:, :, t], rtol=1e-10, atol=1e-18)
        assert np.allclose(Pp[:, :, t], (np.eye(6) - L[:, :, t]) @ Pm[:, :, t], rtol=1e-8, atol=1e-18)
        assert np.array_equal(Pp[:, :, t], Pp[:, :, t].T)
        assert (np.diag(Pp[:, :, t]) < np.diag(Pm[:, :, t])).all() and (np.diag(Pp[:, :, t]) < RHO ** 2).all()
        if t < T - 1:
            assert np.allclose(Pm[:, :, t + 1], A[t] @ Pp[:, :, t] @ A[t].T + W, rtol=1e-12, atol=1e-20)
    for bad in (np.zeros(6), np.r_[RHO[:5], -1.0], np.r_[RHO[:5], np.nan], RHO[:5]):
        with pytest.raises(ValueError, match="rho"):
            batch.filter_gains(None, xo, uo, S0, SIGMA, bad, jac=(A[:T - 1], B[:T - 1]))


def test_host_checker_with_zero_gains_estimates_nothing():
    """L = 0, no ehat0, g4 (a rollout, so c = 0): the estimate stays exactly 0 and u = u_opt, so the members run open loop"""
    from test_gpu_covariance import g4_jacobians
    from test_gpu_ensemble import deltas
    from test_gpu_lqg import lqg_loop
    g, mdl, (A, B, xp) = g4_jacobians()
    T, M = 40, 3
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    assert np.array_equal(xp[:T - 1], xo[:, 1:].T)
    xx, uu, xhat, err = lqg_loop(mdl, xo, uo, KK, np.zeros((6, 6, T)), (A[:T - 1], B[:T - 1], xp[:T - 1]), xo[:, 0] + deltas(M))
    assert np.array_equal(xhat, np.broadcast_to(xo, (M, 6, T)))
    assert np.array_equal(uu[:, :, :T - 1], np.broadcast_to(uo[:, :T - 1], (M, 2, T - 1)))
    assert np.array_equal(err, xx - xo[None]) and np.abs(err).max() > 0.1


@pytest.mark.parametrize("s", [0.1, 1.0])
def test_host_checker_against_the_filters_own_covariance(s):
    """The Monte Carlo of the issue on the CPU with the generator's own draws (seed MC_SEED): the first 200 samples of g4 with
    its own gains, 2048 members with deltas default_rng(3).normal(size=(M,6)) * DELTA_SCALE * s, SIGMA, rho = 0.1 DELTA_SCALE,
    the filter built on the population spread.  At s = 0.1 the sampled covariance and mean of e = dx - e^+ agree with P^+ and
    0 within sampling error (z_cov, z_mean <= 5; the expected maximum of that many standard normals is about 3.7); at s = 1.0
    they do not (z_cov >= 15).  Measured here: s = 0.1: z_cov 3.49, z_mean 3.51; s = 1.0: z_cov 2.83e+03, z_mean 102."""
    from aircraftoptimalcontrol_amd import mpc
    from test_gpu_covariance import MC_M, MC_SEED, MC_T, g4_jacobians, mc_members
    from test_gpu_ensemble import SIGMA
    from test_gpu_lqg import RHO, lqg_loop, mc_gains, mc_z
    g, mdl, (A, B, xp) = g4_jacobians()
    T, M = MC_T, MC_M
    xo, uo, KK, L, P_post = mc_gains(s)
    d = mc_members(s)[0]
    dist = np.zeros((M, 6, T))
    for t in range(T - 1):
        dist[:, :, t] = mpc.noise_draws(MC_SEED, t, 0, M, SIGMA)
    meas = np.stack([mpc.noise_draws(MC_SEED, t, 0, M, RHO, 1) for t in range(T)], axis=2)
    _, _, _, err = lqg_loop(mdl, xo, uo, KK, L, (A[:T - 1], B[:T - 1], xp[:T - 1]), xo[:, 0] + d, None, dist, meas)
    zc, zm = mc_z(err, P_post)
    rms = np.sqrt((err ** 2).mean(axis=(0, 2)))
    print("s = %g: z_cov = %.3g, z_mean = %.3g, rms e / rho = %s" % (s, zc, zm, np.round(rms / RHO, 3)))
    if s == 0.1:
        assert zc <= 5 and zm <= 5, (zc, zm)
    else:
        assert zc >= 15, zc


def test_the_reference_gap_is_the_one_the_gpu_tolerance_is_built_on():
    """REF_GAP of tests/test_gpu_lqg.py is the checker's own rounding (fp64 against np.longdouble in the estimator), re-measured
    here on the cases that set it: nothing measured exceeds the constant, and the constant is not padded beyond 2x what is
    measured.  (A float32 rounding flip of the plant between the two checkers would show as a gap near 1e-7.)"""
    from test_gpu_lqg import REF_GAP, reference_gap
    gap = reference_gap()
    print("checker fp64 against long double: %.3g (REF_GAP %.3g)" % (gap, REF_GAP))
    assert 0.5 * REF_GAP <= gap <= REF_GAP
