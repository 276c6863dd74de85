"""aoc_track_ensemble_limited / batch.track_ensemble(u_min=, u_max=, u_rate=): actuator limits and rate limits in the
closed loop of the tracking ensembles.

The checker is host_loop_limited of tests/test_limits_abi.py: host_loop of tests/test_gpu_ensemble.py with the selection
of include/aoc.h between forming the demand and stepping the plant.  The limits are selections, not arithmetic, so the
bar is bit-identity: with infinite limits against the calls without limits, with finite ones against the checker.  Unless
a test says otherwise the ensemble is B = 322 members on two nominals in groups of 192: the last tile is partial and a
group boundary falls mid-array.  The limits are the fixed ones of tests/test_limits_abi.py."""
import numpy as np
import pytest

from test_gpu_ensemble import SIGMA, ST_NAN, ST_VNONPOS, _g4, _problem, _two_nominals, deltas, host_cost, numpy_stats
from test_limits_abi import INF2, U_MAX, U_MIN, U_RATE, host_loop_limited

pytestmark = pytest.mark.gpu

B, MPO = 322, 192
SHARED = ("stats", "status", "max_dx", "max_du", "cost", "final_dx", "first_bad")
SHARED_TRAJ = SHARED + ("xx_reg", "uu_reg", "dist")
Q3 = (0.05, 0.5, 0.95)
KINDS = dict(mag=(U_MIN, U_MAX, INF2), rate=(-INF2, INF2, U_RATE), both=(U_MIN, U_MAX, U_RATE))
NONE = dict(u_min=-INF2, u_max=INF2, u_rate=INF2)


def _kw(kind):
    lo, hi, rate = KINDS[kind]
    return dict(u_min=lo, u_max=hi, u_rate=rate)


def _setup(T):
    """two nominals cut to T samples, the problem, the gains of the fixture for both, and the members"""
    g, mdl, _ = _g4()
    XO, UO = _two_nominals(g)
    XO, UO = XO[:, :, :T], UO[:, :, :T]
    KK = np.stack([g["KK"][:, :, :T]] * 2)
    bp = _problem(dict(g, xx_opt=XO[0]))
    return g, mdl, bp, XO, UO, KK, dict(delta=deltas(B), KK=KK, members_per_opt=MPO)


def _checker(g, mdl, XO, UO, KK, d, sel, kind, dist=None):
    """host_loop_limited for the members sel (global indices) of the two groups -> the checker's tuple, rows in sel's order"""
    lo, hi, rate = KINDS[kind]
    sel = np.asarray(sel)
    parts = []
    for k in range(2):
        m = sel[sel // MPO == k]
        if len(m):
            parts.append(host_loop_limited(mdl, XO[k], UO[k], KK[k], XO[k][:, 0] + d[m], lo, hi, rate,
                                           None if dist is None else dist[m]))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(7))


@pytest.mark.parametrize("variant", ["plain", "noise", "float32"])
@pytest.mark.parametrize("mode", ["stats", "envelope", "histogram"])
def test_infinite_limits_change_no_bit(mode, variant):
    """lo = -inf, hi = +inf, rate = +inf: every output shared with the calls without limits has their bits, in all three
    modes, with and without noise and with float32 state storage; sat is 0 / T / +0.0 and sat_count all zero."""
    from aircraftoptimalcontrol_amd import batch
    T = 33
    g, mdl, bp, XO, UO, KK, kw = _setup(T)
    if variant == "noise":
        kw.update(sigma=SIGMA, seed=20261019)
    if variant == "float32":
        kw.update(f32=True)
    if mode == "envelope":
        kw.update(envelope=True)
    if mode == "histogram":
        kw.update(quantiles=Q3)
    for traj in (True, False):
        if variant == "float32" and not traj:
            continue
        old = batch.track_ensemble(bp, XO, UO, trajectories=traj, **kw)
        r = batch.track_ensemble(bp, XO, UO, trajectories=traj, **kw, **NONE)
        assert "sat" not in old and "sat_count" not in old and "frac_cut" not in old["summary"][0]
        for k in (SHARED_TRAJ if traj else SHARED):
            assert np.array_equal(r[k], old[k]), (k, traj)
        if mode != "stats":
            raw = lambda x: np.stack([e["raw"] for e in x["envelope"]])
            assert np.array_equal(raw(r), raw(old))
        if mode == "histogram":
            assert np.array_equal(np.stack(r["hist"]), np.stack(old["hist"]))
            assert np.array_equal(np.stack(r["bins"]), np.stack(old["bins"]))
        assert r["sat"].shape == (B, 6) and not r["sat"][:, 0:2].any() and (r["sat"][:, 2:4] == T).all()
        assert not r["sat"][:, 4:6].any() and not np.signbit(r["sat"][:, 4:6]).any()
        assert len(r["sat_count"]) == 2
        for c in r["sat_count"]:
            assert c.shape == (T, 2) and c.dtype == np.int32 and not c.any()
        assert all(np.array_equal(sm["frac_cut"], [0.0, 0.0]) for sm in r["summary"])


@pytest.mark.parametrize("T", [3, 4, 16, 17, 18, 33, 200])
@pytest.mark.parametrize("kind", ["mag", "rate", "both"])
def test_parity_with_the_host_loop_bit_for_bit(kind, T):
    """x_reg, u_reg, the sixteen statistics (numpy_stats + host_cost on the checker's trajectories) and sat equal
    host_loop_limited bit for bit, without noise and — the device's own dist handed to the checker — with it.  T = 3: the
    rate limit acts at t = 1 alone; 16, 17, 18: the edges of the 16-record prefetch block.  All members at T <= 33, six of
    the first group and two of the second at T = 200."""
    from aircraftoptimalcontrol_amd import batch
    g, mdl, bp, XO, UO, KK, kw = _setup(T)
    sel = np.arange(B) if T <= 33 else np.array([0, 1, 63, 64, 100, 191, 192, 321])
    grp = sel // MPO
    for noise in (False, True):
        nkw = dict(sigma=SIGMA, seed=20261019) if noise else {}
        r = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw, **nkw, **_kw(kind))
        assert r["dist"].any() == noise
        xx, uu, vv, ncut, first, maxd, cut = _checker(g, mdl, XO, UO, KK, kw["delta"], sel, kind, r["dist"] if noise else None)
        assert np.array_equal(r["xx_reg"][sel], xx), (noise, "xx")
        assert np.array_equal(r["uu_reg"][sel], uu), (noise, "uu")
        cost = np.concatenate([host_cost(g["QQt"], g["RRt"], g["QQT"], xx[grp == k], uu[grp == k], XO[k], UO[k]) for k in range(2)])
        assert np.array_equal(r["stats"][sel], numpy_stats(xx, uu, XO[grp], UO[grp], cost)), (noise, "stats")
        assert np.array_equal(r["sat"][sel], np.concatenate([ncut, first, maxd], axis=1)), (noise, "sat")
        if T == 200 and kind != "rate" and not noise:
            assert ncut[:, 0].any()                                  # the limits bite among the members looked at
        so = batch.track_ensemble(bp, XO, UO, **kw, **nkw, **_kw(kind))
        for k in SHARED + ("sat",):
            assert np.array_equal(so[k], r[k]), (noise, k)


@pytest.fixture(scope="module")
def both33():
    """T = 33 under both limits, no noise: the setup and the checker's cut flags of all 322 members, computed once"""
    T = 33
    g, mdl, bp, XO, UO, KK, kw = _setup(T)
    chk = _checker(g, mdl, XO, UO, KK, kw["delta"], np.arange(B), "both")
    return T, bp, XO, UO, kw, chk


def test_sat_count_is_the_count_over_the_cut_flags(both33):
    """sat_count of each optimum equals NumPy's count over the checker's cut flags of its members — 192 and 130: the 62
    lanes that replicate member 321 add nothing —, is zero at sample T-1, has the same bits with and without trajectories
    and on a second call, and frac_cut is the share of members with a cut."""
    from aircraftoptimalcontrol_amd import batch
    T, bp, XO, UO, kw, chk = both33
    cut, ncut = chk[6], chk[3]
    assert cut[:MPO].any() and cut[MPO:].any() and not (chk[0][:, 2] <= 0).any()
    r = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw, **_kw("both"))
    assert (r["first_bad"] == T).all()
    want = [cut[:MPO].sum(axis=0).T, cut[MPO:].sum(axis=0).T]
    for k in range(2):
        assert r["sat_count"][k].dtype == np.int32 and np.array_equal(r["sat_count"][k], want[k]), k
        assert not r["sat_count"][k][T - 1].any()
        n = MPO if k == 0 else B - MPO
        assert np.array_equal(r["summary"][k]["frac_cut"], (ncut[k * MPO:k * MPO + n] > 0).sum(axis=0) / n)
    assert r["sat_count"][1].max() <= B - MPO
    again = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw, **_kw("both"))
    so = batch.track_ensemble(bp, XO, UO, **kw, **_kw("both"))
    for other in (again, so):
        for k in range(2):
            assert np.array_equal(other["sat_count"][k], r["sat_count"][k])
        assert np.array_equal(other["sat"], r["sat"]) and np.array_equal(other["stats"], r["stats"])


def test_sat_count_of_two_calls_merges_to_the_one_call():
    """One optimum, 322 members, noise on: the calls over members [0,128) and [128,322) with first= merge
    (sat_count_merge) to the one-call counts, and their per-member outputs concatenate to its."""
    from aircraftoptimalcontrol_amd import batch
    T = 33
    g, mdl, bp, XO, UO, KK, _ = _setup(T)
    d = deltas(B)
    run = lambda sl, **kw: batch.track_ensemble(bp, XO[0], UO[0], delta=d[sl], KK=KK[0], sigma=SIGMA, seed=20261019,
                                                **_kw("both"), **kw)
    one, a, b = run(slice(0, B)), run(slice(0, 128), first=0), run(slice(128, B), first=128)
    assert one["sat_count"][0].any()
    assert np.array_equal(batch.sat_count_merge(a["sat_count"][0], b["sat_count"][0]), one["sat_count"][0])
    for k in ("stats", "status", "sat"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), one[k]), k


def test_a_bad_member_among_good_ones():
    """One member starts at V <= 0, one has a NaN in its x0, among 62 ordinary ones: both are flagged with first_bad = 0,
    the others are bit-identical to a call without the two, sat_count is the count over the others alone (a member is
    missing from its first_bad on), and the NaN member's demand is never counted as cut."""
    from aircraftoptimalcontrol_amd import batch
    T = 33
    g, mdl, _ = _g4()
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    bp = _problem(dict(g, xx_opt=xo))
    d = deltas(64)
    run = lambda dd: batch.track_ensemble(bp, xo, uo, delta=dd, KK=KK, trajectories=True, **_kw("both"))
    clean = run(d)
    d2 = d.copy()
    d2[17] = [0, 0, -40, 0, 0, 0]
    d2[40, 4] = np.nan
    r = run(d2)
    assert xo[2, 0] - 40 < 0
    assert r["status"][17] & ST_VNONPOS and r["first_bad"][17] == 0
    assert r["status"][40] & ST_NAN and r["first_bad"][40] == 0
    others = np.setdiff1d(np.arange(64), [17, 40])
    for k in ("xx_reg", "uu_reg", "stats", "status", "sat"):
        assert np.array_equal(r[k][others], clean[k][others]), k
    assert (clean["first_bad"] == T).all() and not clean["status"].any()
    lo, hi, rate = KINDS["both"]
    cut = host_loop_limited(mdl, xo, uo, KK, xo[:, 0] + d, lo, hi, rate)[6]
    assert cut[17].any() or cut[40].any() or cut[others].any()
    assert np.array_equal(clean["sat_count"][0], cut.sum(axis=0).T)
    assert np.array_equal(r["sat_count"][0], cut[others].sum(axis=0).T)
    assert np.isnan(r["uu_reg"][40, :, :T - 1]).all()               # a NaN demand stays NaN ...
    assert not r["sat"][40, 0:2].any() and (r["sat"][40, 2:4] == T).all() and np.isnan(r["sat"][40, 4:6]).all()   # ... uncut
    assert r["summary"][0]["n_bad"] == 2


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
def test_the_limits_hold(noise):
    """Under both limits every input sample lies in [lo, hi] and, from sample 1 on, in [fl(u_{t-1} - s), fl(u_{t-1} + s)]
    with s = rate * dt, and some samples sit on each kind of bound."""
    from aircraftoptimalcontrol_amd import batch
    T = 200
    g, mdl, bp, XO, UO, KK, kw = _setup(T)
    if noise:
        kw.update(sigma=SIGMA, seed=20261019)
    r = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw, **_kw("both"))
    u = r["uu_reg"][:, :, :T - 1]
    lo, hi, s = U_MIN[None, :, None], U_MAX[None, :, None], (U_RATE * np.float64(g["dt"]))[None, :, None]
    assert ((u >= lo) & (u <= hi)).all()
    assert ((u[:, :, 1:] >= u[:, :, :-1] - s) & (u[:, :, 1:] <= u[:, :, :-1] + s)).all()
    assert (u == lo).any() and (u == hi).any()
    assert (u[:, :, 1:] == u[:, :, :-1] - s).any() and (u[:, :, 1:] == u[:, :, :-1] + s).any()
    assert not r["uu_reg"][:, :, T - 1].any()


def test_envelope_and_histogram_under_limits():
    """The envelope and the counts are NumPy's reductions of the device's own limited trajectories (the checkers of
    tests/test_gpu_envelope.py and tests/test_gpu_histogram.py), and the envelope's du lies inside [lo - u_opt, hi - u_opt]."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_envelope import _check_against_own_trajectories, _check_views
    from test_gpu_histogram import _assert_sums, _check
    T = 33
    g, mdl, bp, XO, UO, KK, kw = _setup(T)
    kw.update(sigma=SIGMA, seed=20261019, **_kw("both"))
    traj = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw)
    e = batch.track_ensemble(bp, XO, UO, trajectories=True, envelope=True, **kw)
    _check_against_own_trajectories(e, XO, UO, "limited envelope")
    _check_views(e)
    for k in SHARED_TRAJ + ("sat",):
        assert np.array_equal(e[k], traj[k]), k
    for k in range(2):
        assert np.array_equal(e["sat_count"][k], traj["sat_count"][k])
        env = e["envelope"][k]
        assert (env["min_du"][:, :T - 1] >= np.subtract(U_MIN[:, None], UO[k][:, :T - 1])).all()
        assert (env["max_du"][:, :T - 1] <= np.subtract(U_MAX[:, None], UO[k][:, :T - 1])).all()
    assert any((e["envelope"][k]["min_du"][:, :T - 1] == np.subtract(U_MIN[:, None], UO[k][:, :T - 1])).any() for k in range(2))
    h = batch.track_ensemble(bp, XO, UO, quantiles=Q3, **kw)             # two passes: the envelope call, then the counts
    hist = _check(h, traj, XO, UO, T, "limited histogram")
    _assert_sums(hist, np.stack([x["n"] for x in h["envelope"]]), T)
    assert np.array_equal(np.stack([x["raw"] for x in h["envelope"]]), np.stack([x["raw"] for x in e["envelope"]]))
    for k in SHARED + ("sat",):
        assert np.array_equal(h[k], traj[k]), k
    bins = np.stack(h["bins"])
    h1 = batch.track_ensemble(bp, XO, UO, trajectories=True, quantiles=Q3, bins=bins, **kw)   # one pass, the caller's bins
    assert "envelope" not in h1 and np.array_equal(np.stack(h1["hist"]), hist)
    for k in SHARED_TRAJ + ("sat",):
        assert np.array_equal(h1[k], traj[k]), k
    for k in range(2):
        assert np.array_equal(h1["sat_count"][k], traj["sat_count"][k]) and np.array_equal(h["sat_count"][k], traj["sat_count"][k])


def test_example_prints_limits_and_frac_cut(tmp_path):
    """examples/run_tracking_ensemble.py as a process with the three flags: the JSON line's frac_cut is that of
    batch.track_ensemble for the same seeded members, and its limits are the flags."""
    import json
    from test_gpu_drivers import _run
    from test_gpu_ensemble import DELTA_SCALE
    from aircraftoptimalcontrol_amd import batch, problems
    g, _, _ = _g4()
    T = 200
    xo, uo = g["xx_opt"][:, :T], g["uu_opt"][:, :T]
    np.save(tmp_path / "xx_star.npy", xo)
    np.save(tmp_path / "uu_star.npy", uo)
    out = _run("run_tracking_ensemble.py", "--data", tmp_path, "--members", 1000, "--seed", 5, "--dt", float(g["dt"]),
               "--u-min", *U_MIN, "--u-max", *U_MAX, "--u-rate", *U_RATE)
    line = json.loads(out.strip().split("\n")[-1])
    assert line["members"] == 1000 and line["T"] == T
    assert line["limits"] == dict(u_min=U_MIN.tolist(), u_max=U_MAX.tolist(), u_rate=U_RATE.tolist())
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    d = np.random.default_rng(5).normal(size=(1000, 6)) * DELTA_SCALE
    r = batch.track_ensemble(bp, xo, uo, delta=d, seed=5, u_min=U_MIN, u_max=U_MAX, u_rate=U_RATE)
    assert np.array_equal(np.asarray(line["frac_cut"]), r["summary"][0]["frac_cut"])
    assert 0 < r["summary"][0]["frac_cut"][0] < 1
    assert line["left_the_domain"] == r["summary"][0]["n_bad"]
    for name, v in r["summary"][0]["cost"].items():
        assert np.array_equal(np.asarray(line["cost"][name]), v), name
