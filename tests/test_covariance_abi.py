"""CPU-side checks of aoc_track_covariance: the ABI revision and the struct sizes are what they were, the new symbols are
declared, exported and bound, every argument error is reported with its reason before anything touches a device, the
scratch query; the host checker of tests/test_gpu_covariance.py against a Monte Carlo of the oracle's own closed loop; and
batch.covariance_moments / batch.histogram_bins_predicted on hand-made records."""
import ctypes as C

import numpy as np
import pytest

from aircraftoptimalcontrol_amd import _lib

REC = 56 * 8   # bytes of scratch per (optimum, sample)


def _prob(T=10):
    p = _lib.Problem()
    p.B, p.T = 0, T          # B is not read
    return p


def test_abi_revision_struct_sizes_and_symbols():
    _lib.build_library()
    lib = _lib.lib()
    assert lib.aoc_abi_version() == _lib.AOC_ABI_VERSION == 5
    assert C.sizeof(_lib.Model) == 72
    assert C.sizeof(_lib.Problem) == 72 + 76 * 8 + 32 + 16
    assert C.sizeof(_lib.Params) == 48
    assert C.sizeof(_lib.Tuning) == 104
    assert C.sizeof(_lib.MpcNoise) == 64
    assert _lib.AOC_COV_NREC == 32 and _lib.AOC_ENV_NREC == 44 and _lib.AOC_ENS_NSTAT == 16
    for name in ("aoc_track_covariance", "aoc_track_covariance_scratch_bytes"):
        assert name in _lib.SYMBOLS and getattr(lib, name)
    hdr = open(_lib._HDR).read()
    assert "#define AOC_COV_NREC 32" in hdr and "#define AOC_ABI_VERSION 5" in hdr
    assert "size_t aoc_track_covariance_scratch_bytes(int32_t n_opt, int32_t T);" in hdr
    assert len(_lib.SYMBOLS["aoc_track_covariance"][1]) == 10
    # the entry points before it keep their argument lists
    assert len(_lib.SYMBOLS["aoc_track_ensemble"][1]) == 11
    assert len(_lib.SYMBOLS["aoc_track_ensemble_envelope"][1]) == 14
    assert len(_lib.SYMBOLS["aoc_track_ensemble_histogram"][1]) == 15


def test_scratch_query():
    """one private record per optimum and sample; geometry the call would refuse asks for nothing"""
    q = _lib.lib().aoc_track_covariance_scratch_bytes
    assert q(1, 3) == 3 * REC
    assert q(1, 1000) == 1000 * REC and q(70, 33) == 70 * 33 * REC
    assert q(1024, 1000) == 1024 * 1000 * REC
    assert q(1 << 20, 1 << 20) == (1 << 40) * REC          # no 32-bit product on the way
    assert q(0, 10) == 0 and q(-1, 10) == 0 and q(1, 2) == 0 and q(1, 0) == 0 and q(1, -5) == 0


def test_argument_errors_carry_a_reason():
    lib = _lib.lib()
    big = 1 << 40

    def call(p, n_opt=1, nominal=16, mean0=None, Sigma0=None, noise=None, pred=16, status=None, scratch=16, scratch_bytes=big):
        return lib.aoc_track_covariance(C.byref(p) if p is not None else None, n_opt, nominal, mean0, Sigma0, noise, pred,
                                        status, scratch, scratch_bytes)
    need = lib.aoc_track_covariance_scratch_bytes(2, 10)
    assert need == 2 * 10 * REC
    cases = [
        (dict(p=None), b"aoc_problem is NULL"),
        (dict(p=_prob(), nominal=None), b"nominal is NULL"),
        (dict(p=_prob(), pred=None), b"pred is NULL"),
        (dict(p=_prob(), n_opt=0), b"n_opt = 0"),
        (dict(p=_prob(), n_opt=-3), b"n_opt = -3"),
        (dict(p=_prob(T=2)), b"T = 2"),
        (dict(p=_prob(T=0)), b"T = 0"),
        (dict(p=_prob(), scratch=None), b"scratch is NULL"),
        (dict(p=_prob(), scratch=24), b"16-byte aligned"),
        (dict(p=_prob(), n_opt=2, scratch_bytes=need - 1), b"scratch_bytes = %d, need %d" % (need - 1, need)),
        (dict(p=_prob(), scratch_bytes=0), b"scratch_bytes = 0"),
    ]
    for kw, reason in cases:
        # leave another reason behind first, so that an error return without a new reason shows
        q = _lib.Problem()
        q.B, q.T, q.ref = 4, 2, 1
        assert lib.aoc_traj_cost(C.byref(q), 1, 1, 1, 1) == -1 and b"T = 2 " in lib.aoc_last_hip_error() + b" "
        assert call(**kw) == -1, kw
        msg = lib.aoc_last_hip_error()
        assert msg.startswith(b"aoc_track_covariance: ") and reason in msg, (kw, msg)
    # and a neighbour still names itself
    assert lib.aoc_track_ensemble(C.byref(_prob()), 1, 64, None, 1, None, None, None, None, 1, None) == -1
    assert lib.aoc_last_hip_error().startswith(b"aoc_track_ensemble: ")


def test_the_reference_gap_is_the_one_the_gpu_tolerance_is_built_on():
    """REF_GAP of tests/test_gpu_covariance.py is the checker's own rounding (fp64 against np.longdouble), re-measured here on
    the sizes that set it: nothing measured exceeds the constant, and the constant is not padded beyond 2x what is measured."""
    from test_gpu_covariance import REF_GAP, reference_gap
    gap = reference_gap()
    print("checker fp64 against long double: %.3g (REF_GAP %.3g)" % (gap, REF_GAP))
    assert 0.5 * REF_GAP <= gap <= REF_GAP


def test_host_checker_defects_are_zero_on_a_rollout():
    """g4's optimum is a rollout of the plant: c_t = step(x_opt_t, u_opt_t) - x_opt_{t+1} is exactly 0, so with mean0 = 0 the
    predicted mean stays exactly 0; and with no Sigma0 and no noise so does the covariance."""
    from test_gpu_covariance import g4_jacobians, numpy_covariance
    g, _, jac = g4_jacobians()
    assert np.array_equal(jac[2], g["xx_opt"][:, 1:].T)
    rec = numpy_covariance(jac, g["xx_opt"], g["KK"])
    assert rec.shape == (g["xx_opt"].shape[1], 32) and not rec.any()


@pytest.mark.parametrize("s", [0.1, 1.0])
def test_host_checker_against_a_monte_carlo_of_the_oracle(s):
    """The Monte Carlo of the issue on the CPU: the first 200 samples of g4 with its own gains, 2048 members with deltas
    default_rng(3).normal(size=(M,6)) * DELTA_SCALE * s, SIGMA, noise seed 7, population moments Sigma0 =
    diag((DELTA_SCALE s)^2), mean0 = 0.  At s = 0.1 the sampled moments agree with the linear prediction within sampling
    error (z_cov, z_mean <= 5); at s = 1.0 they do not (z_cov >= 15): the comparison separates the regimes.
    Measured here: s = 0.1: z_cov 2.24, z_mean 2.14; s = 1.0: z_cov 48.5, z_mean 22.0."""
    from aircraftoptimalcontrol_amd import mpc
    from test_gpu_covariance import MC_M, MC_SEED, MC_T, SIGMA, g4_jacobians, host_loop, mc_members, numpy_covariance, z_scores
    g, mdl, (A, B, xp) = g4_jacobians()
    T, M = MC_T, MC_M
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    d, m0, S0 = mc_members(s)
    dist = np.zeros((M, 6, T))
    for t in range(T - 1):
        dist[:, :, t] = mpc.noise_draws(MC_SEED, t, 0, M, SIGMA)
    xx, _ = host_loop(mdl, xo, uo, KK, xo[:, 0] + d, dist)
    dx = xx - xo[None]
    mean = dx.mean(axis=0)                                                             # (6,T)
    S = np.einsum("mit,mjt->ijt", dx, dx) / M - mean[:, None, :] * mean[None, :, :]
    rec = numpy_covariance((A[:T - 1], B[:T - 1], xp[:T - 1]), xo, KK, m0, S0, SIGMA)
    from aircraftoptimalcontrol_amd import batch
    m, P, _, _ = batch.covariance_moments(rec)
    zc, zm = z_scores(S, mean, P, m, M)
    print("s = %g: z_cov = %.2f, z_mean = %.2f" % (s, zc, zm))
    if s == 0.1:
        assert zc <= 5 and zm <= 5, (zc, zm)
    else:
        assert zc >= 15, zc


def test_end_bins_of_the_predicted_range_on_the_host_loop():
    """Bins of mean -+ 6 std from the checker's prediction, the oracle's closed loop binned under them with NumPy (256 members,
    s = 0.1, T = 200): the two end bins together hold at most 1 % of any (sample, state channel)."""
    from aircraftoptimalcontrol_amd import batch, mpc
    from test_gpu_covariance import MC_SEED, MC_T, SIGMA, g4_jacobians, host_loop, mc_members, numpy_covariance
    g, mdl, (A, B, xp) = g4_jacobians()
    T, M = MC_T, 256
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    d, m0, S0 = mc_members(0.1, M)
    dist = np.zeros((M, 6, T))
    for t in range(T - 1):
        dist[:, :, t] = mpc.noise_draws(MC_SEED, t, 0, M, SIGMA)
    xx, uu = host_loop(mdl, xo, uo, KK, xo[:, 0] + d, dist)
    rec = numpy_covariance((A[:T - 1], B[:T - 1], xp[:T - 1]), xo, KK, m0, S0, SIGMA)
    bins = batch.histogram_bins_predicted(rec, 6.0)[0]                                 # (T,8,2)
    v = np.concatenate([xx - xo[None], uu - uo[None]], axis=1).transpose(2, 1, 0)      # (T,8,M)
    sc = (v - bins[:, :, 0:1]) * bins[:, :, 1:2]
    outside = ((sc < 1.0) | (sc >= 63.0)).mean(axis=-1)                                # share in bins 0 and 63
    outside[T - 1, 6:] = 0.0                                                           # no input at the last sample
    print("largest share of the two end bins: %.4f" % outside.max())
    assert outside.max() <= 0.01


def _record(T=4):
    rng = np.random.default_rng(1)
    raw = rng.normal(size=(T, 32))
    L = rng.normal(size=(T, 6, 6))
    P = L @ L.transpose(0, 2, 1)
    iu = np.triu_indices(6)
    raw[:, 6:27] = P[:, iu[0], iu[1]]
    raw[:, 29], raw[:, 30], raw[:, 31] = 4.0, -1.0, 9.0
    raw[T - 1, 27:] = 0.0
    return raw, P


def test_covariance_moments_unpacks_the_record():
    from aircraftoptimalcontrol_amd import batch
    raw, P = _record()
    T = raw.shape[0]
    mean_dx, cov_dx, mean_du, cov_du = batch.covariance_moments(raw)
    assert mean_dx.shape == (6, T) and cov_dx.shape == (6, 6, T) and mean_du.shape == (2, T) and cov_du.shape == (2, 2, T)
    assert np.array_equal(mean_dx, raw[:, 0:6].T) and np.array_equal(mean_du, raw[:, 27:29].T)
    assert np.array_equal(cov_dx, P.transpose(1, 2, 0)) and np.array_equal(cov_dx, cov_dx.transpose(1, 0, 2))
    assert np.array_equal(cov_du[:, :, 0], [[4.0, -1.0], [-1.0, 9.0]])
    assert not mean_du[:, T - 1].any() and not cov_du[:, :, T - 1].any()               # sample T-1: no input
    assert cov_dx[1, 2, 0] == raw[0, 6 + 7] and cov_dx[5, 5, 1] == raw[1, 26]          # the envelope's order of the triangle
    with pytest.raises(ValueError):
        batch.covariance_moments(raw[:, :31])
    with pytest.raises(ValueError):
        batch.covariance_moments(raw[None])


def test_histogram_bins_predicted_on_hand_made_records():
    from aircraftoptimalcontrol_amd import batch
    raw, P = _record()
    T = raw.shape[0]
    raw[0, 0], raw[0, 6] = 2.0, 0.25                    # channel 0 at sample 0: mean 2, std 0.5
    raw[1, 1], raw[1, 6 + 6] = -1.0, 0.0                # std = 0
    raw[1, 2], raw[1, 6 + 11] = 3.0, np.nan             # std NaN, mean finite
    raw[2, 3], raw[2, 6 + 15] = np.nan, 1.0             # mean NaN
    raw[2, 4], raw[2, 6 + 18] = np.inf, np.inf          # neither finite
    raw[2, 5], raw[2, 26] = 1.0, -1e-30                 # a variance rounded below 0: sqrt is NaN
    raw[3, 0], raw[3, 6] = 0.5, 1e-320                  # std so small that 64 / (2 k std) is still finite or overflows
    bins = batch.histogram_bins_predicted(raw, 6.0)
    assert bins.shape == (1, T, 8, 2) and np.isfinite(bins).all()
    b = bins[0]
    assert np.array_equal(b[0, 0], [2.0 - 6.0 * 0.5, 64.0 / (2 * 6.0 * 0.5)])
    assert np.array_equal(b[1, 1], [-1.0, 0.0]) and np.array_equal(b[1, 2], [3.0, 0.0])
    assert np.array_equal(b[2, 3], [0.0, 0.0]) and np.array_equal(b[2, 4], [0.0, 0.0]) and np.array_equal(b[2, 5], [1.0, 0.0])
    assert b[3, 0, 1] == 0.0 or np.isfinite(b[3, 0, 1])
    # the input channels: std from entries 29 and 31, and (mean = 0, 0) at sample T-1
    assert np.array_equal(b[0, 6], [raw[0, 27] - 6.0 * 2.0, 64.0 / 24.0]) and np.array_equal(b[0, 7], [raw[0, 28] - 18.0, 64.0 / 36.0])
    assert np.array_equal(b[T - 1, 6:], np.zeros((2, 2)))
    # k scales the range; (T,32) and (n_opt,T,32) are both taken
    b3 = batch.histogram_bins_predicted(np.stack([raw, raw]), 3.0)
    assert b3.shape == (2, T, 8, 2) and np.array_equal(b3[1, 0, 0], [2.0 - 1.5, 64.0 / 3.0])
    for bad in (raw[:, :31], raw[None, None]):
        with pytest.raises(ValueError):
            batch.histogram_bins_predicted(bad)
    with pytest.raises(ValueError):
        batch.histogram_bins_predicted(raw, 0.0)
