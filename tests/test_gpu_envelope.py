"""aoc_track_ensemble_envelope / batch.track_ensemble(..., envelope=True): the reduction over the members at every sample.

The checker is NumPy on the trajectories OF THE SAME CALL (tests/test_gpu_ensemble.py pins those to the reference bit for
bit), never the envelope itself: numpy_envelope below.  n, the minima and the maxima do not depend on the order of
reduction and are compared with np.array_equal.

Tolerance of the sums, derived, not measured.  Any order of fp64 addition of N terms is within (N-1) 2^-53 sum|term| of the
exact sum (first order), a product adds at most one rounding; the device and NumPy each carry that, so a sum S over the n
members that count passes iff

    |S_dev - S_np| <= 2 (n + 2) 2^-53 sum|term|,

sum|term| computed per record from the trajectories (numpy_envelope returns it beside the record).
"""
import numpy as np
import pytest

from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem, _two_nominals, deltas

pytestmark = pytest.mark.gpu

NREC = 44
I_MIN = np.r_[1:7, 13:15]
I_MAX = np.r_[7:13, 15:17]
I_SUM = np.r_[17:44]
TRI = [(i, j) for i in range(6) for j in range(i, 6)]
U = 2.0 ** -53


def numpy_envelope(xx, uu, xo, uo, first_bad, group):
    """The record of include/aoc.h with NumPy: trajectories xx (M,6,T), uu (M,2,T) about the nominals xo (n_opt,6,T) or
    (6,T), uo likewise; member b belongs to optimum group[b] and counts at sample t iff t < first_bad[b].
    -> rec (n_opt,T,44), mag (n_opt,T,44): for the sums (17-43) the sum of |term| over the members that count, else 0."""
    xx, uu = np.asarray(xx, dtype=np.float64), np.asarray(uu, dtype=np.float64)
    xo, uo = np.asarray(xo, dtype=np.float64), np.asarray(uo, dtype=np.float64)
    if xo.ndim == 2:
        xo, uo = xo[None], uo[None]
    first_bad, group = np.asarray(first_bad), np.asarray(group)
    n_opt, T = xo.shape[0], xx.shape[2]
    rec, mag = np.zeros((n_opt, T, NREC)), np.zeros((n_opt, T, NREC))
    for k in range(n_opt):
        m = np.flatnonzero(group == k)
        counts = np.arange(T)[None, :] < first_bad[m][:, None]                     # (m,T)
        c3 = counts[:, None, :]
        dx, du = np.subtract(xx[m], xo[k]), np.subtract(uu[m], uo[k])
        rec[k, :, 0] = counts.sum(axis=0)
        rec[k, :, 1:7] = np.where(c3, dx, np.inf).min(axis=0, initial=np.inf).T
        rec[k, :, 7:13] = np.where(c3, dx, -np.inf).max(axis=0, initial=-np.inf).T
        rec[k, :, 13:15] = np.where(c3, du, np.inf).min(axis=0, initial=np.inf).T
        rec[k, :, 15:17] = np.where(c3, du, -np.inf).max(axis=0, initial=-np.inf).T
        rec[k, T - 1, 13:15], rec[k, T - 1, 15:17] = np.inf, -np.inf               # no input at the last sample
        dz = np.where(c3, dx, 0.0)                                                # a member that left contributes nothing
        rec[k, :, 17:23] = dz.sum(axis=0).T
        mag[k, :, 17:23] = np.abs(dz).sum(axis=0).T
        for q, (i, j) in enumerate(TRI):
            p = dz[:, i] * dz[:, j]
            rec[k, :, 23 + q] = p.sum(axis=0)
            mag[k, :, 23 + q] = np.abs(p).sum(axis=0)
    return rec, mag


def sum_bound(n, mag):
    """2 (n + 2) 2^-53 sum|term| per record: n (...,), mag (...,44) -> (...,44)"""
    return 2.0 * (np.asarray(n)[..., None] + 2.0) * U * mag


def assert_record(raw, rec, mag, what=""):
    """raw (…,44) from the device against the checker's rec / mag: n, min, max exactly, the sums within sum_bound"""
    raw = np.asarray(raw)
    assert raw.shape == rec.shape, (what, raw.shape, rec.shape)
    assert np.array_equal(raw[..., 0], rec[..., 0]), (what, "n")
    assert np.array_equal(raw[..., I_MIN], rec[..., I_MIN]), (what, "min")
    assert np.array_equal(raw[..., I_MAX], rec[..., I_MAX]), (what, "max")
    err, bound = np.abs(raw[..., I_SUM] - rec[..., I_SUM]), sum_bound(rec[..., 0], mag)[..., I_SUM]
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("%s: largest sum error %.3e, bound there %.3e" % (what, err[worst], bound[worst]))
    assert np.all(err <= bound), (what, worst, err[worst], bound[worst])


def assert_finite(raw, T):
    """every number of every record is finite — but for the one place where the record itself is defined as the empty set:
    min / max of du at sample T-1 (there is no input there)"""
    raw = np.asarray(raw)
    assert np.array_equal(raw[..., T - 1, 13:15], np.full(raw.shape[:-2] + (2,), np.inf))
    assert np.array_equal(raw[..., T - 1, 15:17], np.full(raw.shape[:-2] + (2,), -np.inf))
    rest = raw.copy()
    rest[..., T - 1, 13:17] = 0.0
    assert np.isfinite(rest).all()


def _raw(r):
    return np.stack([e["raw"] for e in r["envelope"]])


def _check_against_own_trajectories(r, XO, UO, what):
    rec, mag = numpy_envelope(r["xx_reg"], r["uu_reg"], XO, UO, r["first_bad"], r["group"])
    assert_record(_raw(r), rec, mag, what)
    return rec, mag


def _check_views(r):
    """the per-optimum dict is what envelope_moments makes of `raw`"""
    from aircraftoptimalcontrol_amd import batch
    for e in r["envelope"]:
        raw = e["raw"]
        T = raw.shape[0]
        n, mean, cov = batch.envelope_moments(raw)
        assert e["n"].dtype.kind == "i" and np.array_equal(e["n"], raw[:, 0])
        assert np.array_equal(e["min_dx"], raw[:, 1:7].T) and np.array_equal(e["max_dx"], raw[:, 7:13].T)
        assert np.array_equal(e["min_du"], raw[:, 13:15].T) and np.array_equal(e["max_du"], raw[:, 15:17].T)
        assert e["mean_dx"].shape == (6, T) and e["cov_dx"].shape == (6, 6, T)
        assert np.array_equal(e["mean_dx"], mean, equal_nan=True) and np.array_equal(e["cov_dx"], cov, equal_nan=True)
        assert np.array_equal(e["cov_dx"], e["cov_dx"].transpose(1, 0, 2), equal_nan=True)


SHARED = ("stats", "status", "max_dx", "max_du", "cost", "final_dx", "first_bad")
SHARED_TRAJ = SHARED + ("xx_reg", "uu_reg", "dist")


@pytest.mark.parametrize("dense", [False, True], ids=["diag", "dense"])
def test_two_nominals_partial_last_tile(dense):
    """Two nominals, 192 members per optimum, B = 322: the second group is two tiles + two live lanes, and the 62 lanes
    that replicate member 321 must not count (n of group 1 is 130 at every sample).  The envelope equals the checker on the
    call's own trajectories; everything the call shares with aoc_track_ensemble has the same bits; the call without
    trajectories gives the same envelope bit for bit."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_dense import _tracking_weights
    g, _, T = _g4()
    bp = _problem(g, _tracking_weights() if dense else None)
    XO, UO = _two_nominals(g)
    B, mpo = 322, 192
    d = deltas(B)
    KK, _ = batch.tracking_gains(bp, XO, UO)
    r = batch.track_ensemble(bp, XO, UO, delta=d, KK=KK, members_per_opt=mpo, trajectories=True, envelope=True)
    assert len(r["envelope"]) == 2 and _raw(r).shape == (2, T, NREC)
    assert (r["envelope"][0]["n"] == 192).all() and (r["envelope"][1]["n"] == 130).all()
    _check_against_own_trajectories(r, XO, UO, "two nominals, trajectories")
    _check_views(r)
    assert_finite(_raw(r), T)
    old = batch.track_ensemble(bp, XO, UO, delta=d, KK=KK, members_per_opt=mpo, trajectories=True)
    assert "envelope" not in old
    for k in SHARED_TRAJ:
        assert np.array_equal(r[k], old[k], equal_nan=True), k
    so = batch.track_ensemble(bp, XO, UO, delta=d, KK=KK, members_per_opt=mpo, envelope=True)
    assert "xx_reg" not in so
    assert np.array_equal(_raw(so), _raw(r))
    old_so = batch.track_ensemble(bp, XO, UO, delta=d, KK=KK, members_per_opt=mpo)
    for k in SHARED:
        assert np.array_equal(so[k], old_so[k], equal_nan=True), k


@pytest.mark.parametrize("variant", ["float32", "noise", "dense_noise", "dense_float32"])
def test_shared_outputs_keep_their_bits(variant):
    """The remaining instances (float32 state storage, the disturbance, dense weights with either): the outputs shared
    with aoc_track_ensemble are bit-identical, with and without trajectories, and the envelope equals the checker on the
    call's own trajectories (float32 storage holds the states exactly for t >= 1, sample 0 is the fp64 x0)."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_dense import _tracking_weights
    g, _, _ = _g4()
    T, B = 200, 192
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    bp = _problem(dict(g, xx_opt=xo), _tracking_weights() if "dense" in variant else None)
    kw = dict(delta=deltas(B), KK=KK)
    if "noise" in variant:
        kw.update(sigma=SIGMA, seed=20261016)
    if "float32" in variant:
        kw.update(f32=True)
    r = batch.track_ensemble(bp, xo, uo, trajectories=True, envelope=True, **kw)
    old = batch.track_ensemble(bp, xo, uo, trajectories=True, **kw)
    for k in SHARED_TRAJ:
        assert np.array_equal(r[k], old[k]), k
    _check_against_own_trajectories(r, xo, uo, variant)
    kw.pop("f32", None)
    so, old_so = batch.track_ensemble(bp, xo, uo, envelope=True, **kw), batch.track_ensemble(bp, xo, uo, **kw)
    for k in SHARED:
        assert np.array_equal(so[k], old_so[k]), k
    assert np.array_equal(_raw(so), _raw(r))


def test_the_same_call_twice_gives_the_same_bits():
    from aircraftoptimalcontrol_amd import batch
    g, _, T = _g4()
    XO, UO = _two_nominals(g)
    bp = _problem(g)
    run = lambda: _raw(batch.track_ensemble(bp, XO, UO, delta=deltas(1000), KK=np.stack([g["KK"], g["KK"]]), sigma=SIGMA,
                                            seed=7, envelope=True))
    a, b = run(), run()
    assert a.shape == (2, T, NREC) and np.array_equal(a, b)


def test_members_that_left_at_sample_0_never_count():
    """test_leaving_the_domain_is_reported_not_a_fault's ensemble: member 17 starts with V_0 < 0, member 40 with a NaN.
    n = 62 at every sample, every number of the record is finite (no NaN reached a sum, a minimum or a maximum), and the
    record is the checker's on the other 62 members."""
    from aircraftoptimalcontrol_amd import batch
    g, _, T = _g4()
    bp = _problem(g)
    d = deltas(64)
    d[17] = [0, 0, -40, 0, 0, 0]
    d[40, 4] = np.nan
    r = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, KK=g["KK"], trajectories=True, envelope=True)
    assert r["first_bad"][17] == 0 and r["first_bad"][40] == 0
    raw = _raw(r)
    assert (raw[0, :, 0] == 62).all()
    assert_finite(raw, T)
    others = np.setdiff1d(np.arange(64), [17, 40])
    rec, mag = numpy_envelope(r["xx_reg"][others], r["uu_reg"][others], g["xx_opt"], g["uu_opt"], r["first_bad"][others],
                              np.zeros(62, int))
    assert_record(raw, rec, mag, "62 of 64")
    # and the checker with all 64 (the two masked by their first_bad) says the same
    _check_against_own_trajectories(r, g["xx_opt"], g["uu_opt"], "64 with two masked")


def test_members_that_leave_mid_horizon():
    """T = 200 of the g4 optimum with the reference's gains, B = 128, the disturbance of V at sigma = 1 m/s (V_0 = 16 m/s),
    seed 20261016: on the host (host_loop fed mpc.noise_draws) 7 of the 128 members leave the domain, at samples 61, 84,
    101, 122, 130, 148, 165 (with sigma[2] = 0.5 none does, with 2.0 71 do).  The device's draws differ from the host's by
    up to 1e-13 of sigma, so the count is asserted to be neither 0 nor B, not 7 to the member."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, B = 200, 128
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    sigma = SIGMA.copy()
    sigma[2] = 1.0
    r = batch.track_ensemble(_problem(dict(g, xx_opt=xo)), xo, uo, delta=deltas(B), KK=KK, sigma=sigma, seed=20261016,
                             first=0, step0=0, trajectories=True, envelope=True)
    left = int((r["first_bad"] < T).sum())
    print("members that left: %d, at samples %s" % (left, np.sort(r["first_bad"][r["first_bad"] < T]).tolist()))
    assert 0 < left < B
    n = r["envelope"][0]["n"]
    assert n[0] == B and (np.diff(n) <= 0).all() and n[-1] < B
    assert np.array_equal(n, (np.arange(T)[:, None] < r["first_bad"][None, :]).sum(axis=1))
    assert_finite(_raw(r), T)
    _check_against_own_trajectories(r, xo, uo, "mid-horizon leavers")
    _check_views(r)


def test_noise_and_cut_invariance():
    """192 members, T = 200, with the disturbance: one call against two calls (first = 0 / 128) merged with
    batch.envelope_merge — n, min, max exactly, the sums within the bound (each part is a sum of its own, so the merged
    record carries the same first-order bound over the 192 terms)."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, B, seed = 200, 192, 20261016
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    bp = _problem(dict(g, xx_opt=xo))
    d = deltas(B)
    run = lambda sl, **kw: batch.track_ensemble(bp, xo, uo, delta=d[sl], KK=KK, sigma=SIGMA, seed=seed, trajectories=True,
                                                envelope=True, **kw)
    r = run(slice(0, B))
    rec, mag = _check_against_own_trajectories(r, xo, uo, "one call")
    a, b = run(slice(0, 128), first=0), run(slice(128, B), first=128)
    assert (a["envelope"][0]["n"] == 128).all() and (b["envelope"][0]["n"] == 64).all()
    merged = batch.envelope_merge(_raw(a), _raw(b))
    assert_record(merged, rec, mag, "two calls merged")
    whole = _raw(r)
    assert np.array_equal(merged[..., 0], whole[..., 0])
    assert np.array_equal(merged[..., I_MIN], whole[..., I_MIN]) and np.array_equal(merged[..., I_MAX], whole[..., I_MAX])
    assert np.all(np.abs(merged[..., I_SUM] - whole[..., I_SUM]) <= sum_bound(rec[..., 0], mag)[..., I_SUM])


@pytest.mark.slow
def test_size_65536_members():
    """65 536 members x T = 1000, statistics + envelope only: n = 65 536 everywhere.  A second call keeps the trajectories
    on the device and reduces them with torch in fp64: n / min / max exactly, the sums within the bound (evaluated with
    torch as well; the 21 products pair by pair, no temporary beyond one (B, T) array).  At sample 0 the record equals
    NumPy's on x0 - xx_opt[:, 0] with x0 as the host formed it."""
    import torch
    from aircraftoptimalcontrol_amd import batch
    g, _, T = _g4()
    B = 65536
    d = deltas(B)
    bp = _problem(g)
    r = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, KK=g["KK"], envelope=True)
    raw = r["envelope"][0]["raw"]
    assert raw.shape == (T, NREC) and (raw[:, 0] == B).all() and (r["first_bad"] == T).all()
    assert_finite(raw[None], T)
    # sample 0 on the host
    dx0 = (g["xx_opt"][:, 0] + d) - g["xx_opt"][:, 0]
    rec0, mag0 = np.zeros(NREC), np.zeros(NREC)
    rec0[0], rec0[1:7], rec0[7:13] = B, dx0.min(axis=0), dx0.max(axis=0)
    rec0[17:23], mag0[17:23] = dx0.sum(axis=0), np.abs(dx0).sum(axis=0)
    for q, (i, j) in enumerate(TRI):
        p = dx0[:, i] * dx0[:, j]
        rec0[23 + q], mag0[23 + q] = p.sum(), np.abs(p).sum()
    assert raw[0, 0] == B and np.array_equal(raw[0, 1:13], rec0[1:13])
    assert np.all(np.abs(raw[0, I_SUM] - rec0[I_SUM]) <= sum_bound(rec0[0], mag0)[I_SUM])
    # every sample with torch on the device's own trajectories
    t = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, KK=g["KK"], trajectories=True, to_host=False)
    dev = t["xx_reg"].device
    xo, uo = torch.from_numpy(g["xx_opt"]).to(dev), torch.from_numpy(g["uu_opt"]).to(dev)
    dx = t["xx_reg"] - xo[None]                                                    # (B,6,T)
    du = t["uu_reg"] - uo[None]
    del t
    env = torch.from_numpy(raw).to(dev)
    assert torch.equal(env[:, 1:7], dx.amin(dim=0).T) and torch.equal(env[:, 7:13], dx.amax(dim=0).T)
    assert torch.equal(env[:T - 1, 13:15], du.amin(dim=0).T[:T - 1]) and torch.equal(env[:T - 1, 15:17], du.amax(dim=0).T[:T - 1])
    bound = lambda mag: 2.0 * (B + 2.0) * U * mag
    worst = 0.0
    for c in range(6):
        err, lim = (env[:, 17 + c] - dx[:, c].sum(dim=0)).abs(), bound(dx[:, c].abs().sum(dim=0))
        worst = max(worst, float((err / lim).max()))
        assert bool((err <= lim).all()), ("sum", c)
    for q, (i, j) in enumerate(TRI):
        p = dx[:, i] * dx[:, j]                                                    # one (B,T) array
        err, lim = (env[:, 23 + q] - p.sum(dim=0)).abs(), bound(p.abs().sum(dim=0))
        worst = max(worst, float((err / lim).max()))
        assert bool((err <= lim).all()), ("moment", i, j)
    print("65 536 members: largest sum error / bound = %.3e" % worst)


def test_example_saves_the_envelope(tmp_path):
    """examples/run_tracking_ensemble.py --envelope FILE.npz as a process: the file's arrays equal
    batch.track_ensemble(..., envelope=True) for the same seeded members, and the JSON line names the file, n at the last
    sample and the largest band width per state."""
    import json
    from test_gpu_drivers import _run
    from aircraftoptimalcontrol_amd import batch, problems
    g, _, T = _g4()
    np.save(tmp_path / "xx_star.npy", g["xx_opt"])
    np.save(tmp_path / "uu_star.npy", g["uu_opt"])
    f = tmp_path / "tube.npz"
    out = _run("run_tracking_ensemble.py", "--data", tmp_path, "--members", 1000, "--seed", 5, "--dt", float(g["dt"]),
               "--sigma", *SIGMA, "--envelope", f)
    line = json.loads(out.strip().split("\n")[-1])
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    d = np.random.default_rng(5).normal(size=(1000, 6)) * DELTA_SCALE
    e = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, sigma=SIGMA, seed=5, envelope=True)["envelope"][0]
    saved = dict(np.load(f, allow_pickle=False))
    assert sorted(saved) == sorted(e)
    for k, v in e.items():
        assert np.array_equal(saved[k], v, equal_nan=True), k
    assert line["envelope"]["file"] == str(f) and line["envelope"]["n_last"] == int(e["n"][-1]) == 1000
    assert np.array_equal(line["envelope"]["max_width"], (e["max_dx"] - e["min_dx"]).max(axis=1))
    assert line["members"] == 1000 and line["left_the_domain"] == 0
