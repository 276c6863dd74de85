"""aoc_track_ensemble_histogram / batch.track_ensemble(..., quantiles=...): the per-sample histogram over the members.

The checker is NumPy (numpy_histogram of tests/test_histogram_abi.py, the binning rule of include/aoc.h restated) on the
trajectories that the EXISTING aoc_track_ensemble returns (tests/test_gpu_ensemble.py pins those to the reference bit for
bit), never the histogram call itself.  dx and du are formed with the same single subtractions and binned with the same two
operations, counts are integers: everything is compared with np.array_equal.

The tube of the end-to-end test is held to the bound of tests/test_histogram_abi.py: within one bin width (tube_width) of
the order statistic, the bins being those of the envelope's min / max."""
import numpy as np
import pytest

from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem, _two_nominals, deltas
from test_histogram_abi import NBIN, NCH, numpy_histogram

pytestmark = pytest.mark.gpu

SHARED = ("stats", "status", "max_dx", "max_du", "cost", "final_dx", "first_bad")
SHARED_TRAJ = SHARED + ("xx_reg", "uu_reg", "dist")
Q3 = (0.05, 0.5, 0.95)


def _cut(g, T):
    return g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]


def _hist(r):
    return np.stack(r["hist"])


def _raw(r):
    return np.stack([e["raw"] for e in r["envelope"]])


def _assert_sums(hist, n, T):
    """sum over the bins = the members that count: channels 0-5 at every sample, 6-7 at every sample but T-1 (all zero there)"""
    n = np.asarray(n)                                                            # (n_opt,T)
    s = hist.sum(axis=-1)                                                        # (n_opt,T,8)
    assert (hist >= 0).all()
    assert np.array_equal(s[:, :, :6], np.repeat(n[:, :, None], 6, 2))
    assert np.array_equal(s[:, :T - 1, 6:], np.repeat(n[:, :T - 1, None], 2, 2))
    assert not hist[:, T - 1, 6:].any()


def _check(r, old, XO, UO, T, what):
    """the counts of r against NumPy on the trajectories of `old`, a run of aoc_track_ensemble on the same members"""
    bins = np.stack(r["bins"])
    want = numpy_histogram(old["xx_reg"], old["uu_reg"], XO, UO, old["first_bad"], old["group"], bins)
    got = _hist(r)
    assert got.shape == want.shape == (bins.shape[0], T, NCH, NBIN) and got.dtype == np.int32, what
    diff = np.argwhere(got != want)
    assert np.array_equal(got, want), (what, len(diff), diff[:5].tolist())
    return got


@pytest.mark.parametrize("T", [200, 22, 17, 3])
@pytest.mark.parametrize("variant", ["diag", "dense", "diag_noise", "dense_noise"])
def test_two_nominals_partial_last_tile(variant, T):
    """Two nominals, 192 members per optimum, B = 322: the second group is two tiles + two live lanes, and the 62 lanes
    that replicate member 321 must not count.  T = 22 and T = 3 are no multiples of the 16-record block or of the drain
    period (8), 3 is the smallest horizon the call takes; with T = 17 the last sample's bins are record 0 of a block that
    only the stash after the last block of stages puts into LDS."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_dense import _tracking_weights
    g, _, _ = _g4()
    XO, UO = _two_nominals(g)
    XO, UO = XO[:, :, :T], UO[:, :, :T]
    bp = _problem(dict(g, xx_opt=XO[0]), _tracking_weights() if "dense" in variant else None)
    B, mpo = 322, 192
    KK = np.stack([g["KK"][:, :, :T]] * 2)
    kw = dict(delta=deltas(B), KK=KK, members_per_opt=mpo)
    if "noise" in variant:
        kw.update(sigma=SIGMA, seed=20261018)
    r = batch.track_ensemble(bp, XO, UO, quantiles=Q3, **kw)
    old = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw)
    hist = _check(r, old, XO, UO, T, (variant, T))
    n = np.stack([e["n"] for e in r["envelope"]])
    assert (n[0] == 192).all() and (n[1] == 130).all()
    _assert_sums(hist, n, T)
    assert np.array_equal(np.stack(r["bins"]), batch.histogram_bins(_raw(r)))
    for k in SHARED:
        assert np.array_equal(r[k], old[k]), k


@pytest.mark.parametrize("variant", ["float32", "noise", "dense_noise", "dense_float32"])
def test_shared_outputs_keep_their_bits(variant):
    """The histogram call writing everything itself (the caller's bins: no envelope call before it): x_reg, u_reg, dist_out,
    stats and status are bit-identical to aoc_track_ensemble's, with and without trajectories, and hist is the same either
    way."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_dense import _tracking_weights
    g, _, _ = _g4()
    T, B = 200, 192
    xo, uo, KK = _cut(g, T)
    bp = _problem(dict(g, xx_opt=xo), _tracking_weights() if "dense" in variant else None)
    kw = dict(delta=deltas(B), KK=KK)
    if "noise" in variant:
        kw.update(sigma=SIGMA, seed=20261016)
    bins = batch.histogram_bins(_raw(batch.track_ensemble(bp, xo, uo, envelope=True, **kw)))
    tkw = dict(kw, f32=True) if "float32" in variant else kw
    r = batch.track_ensemble(bp, xo, uo, trajectories=True, quantiles=Q3, bins=bins, **tkw)
    old = batch.track_ensemble(bp, xo, uo, trajectories=True, **tkw)
    assert "envelope" not in r
    for k in SHARED_TRAJ:
        assert np.array_equal(r[k], old[k]), k
    so, old_so = batch.track_ensemble(bp, xo, uo, quantiles=Q3, bins=bins, **kw), batch.track_ensemble(bp, xo, uo, **kw)
    for k in SHARED:
        assert np.array_equal(so[k], old_so[k]), k
    assert np.array_equal(_hist(so), _hist(r))
    ref = old if "float32" not in variant else batch.track_ensemble(bp, xo, uo, trajectories=True, **kw)
    _check(r, ref, xo, uo, T, variant)


def test_members_that_left_at_sample_0_never_count():
    """Member 17 starts with V_0 < 0, member 40 with a NaN: 62 count at every sample, and no NaN reaches a bin (a NaN that
    did would land in bin 0 and break the sums)."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T = 40
    xo, uo, KK = _cut(g, T)
    bp = _problem(dict(g, xx_opt=xo))
    d = deltas(64)
    d[17] = [0, 0, -40, 0, 0, 0]
    d[40, 4] = np.nan
    r = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, quantiles=Q3)
    old = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, trajectories=True)
    assert old["first_bad"][17] == 0 and old["first_bad"][40] == 0
    hist = _check(r, old, xo, uo, T, "62 of 64")
    _assert_sums(hist, np.full((1, T), 62), T)
    assert np.isfinite(np.stack(r["bins"])).all() and np.isfinite(np.stack(r["tube"])[:, :, :6]).all()


def test_members_that_leave_mid_horizon():
    """T = 200, B = 128, sigma = 1 m/s on V, seed 20261016 (tests/test_gpu_envelope.py): some members leave mid-horizon.
    The counts follow stats[15]."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, B = 200, 128
    xo, uo, KK = _cut(g, T)
    sigma = SIGMA.copy()
    sigma[2] = 1.0
    bp = _problem(dict(g, xx_opt=xo))
    kw = dict(delta=deltas(B), KK=KK, sigma=sigma, seed=20261016, first=0, step0=0)
    r = batch.track_ensemble(bp, xo, uo, quantiles=Q3, **kw)
    old = batch.track_ensemble(bp, xo, uo, trajectories=True, **kw)
    left = int((old["first_bad"] < T).sum())
    print("members that left: %d" % left)
    assert 0 < left < B
    hist = _check(r, old, xo, uo, T, "mid-horizon leavers")
    n = (np.arange(T)[:, None] < old["first_bad"][None, :]).sum(axis=1)
    assert n[0] == B and n[-1] < B
    _assert_sums(hist, n[None], T)


def test_callers_bins():
    """Corridors narrower than the cloud (outliers in bins 0 and 63), a value exactly on an edge, inv_w = 0, and a NaN in
    bins (bin 0, AOC_OK)."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, B = 22, 128
    xo, uo, KK = _cut(g, T)
    bp = _problem(dict(g, xx_opt=xo))
    d = deltas(B)
    d[5] = [0.25, -0.125, 0.5, 0.0, 0.0625, -0.03125]          # dx at sample 0 is exactly d where x_opt + d - x_opt is exact
    old = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, trajectories=True)
    dx0 = old["xx_reg"][5, :, 0] - xo[:, 0]
    bins = np.zeros((1, T, NCH, 2))
    bins[0, :, :6, 0] = -0.5 * DELTA_SCALE                      # about half a standard deviation either side
    bins[0, :, :6, 1] = 64.0 / DELTA_SCALE
    bins[0, :, 6:, 0], bins[0, :, 6:, 1] = -0.01, 64.0 / 0.02
    # sample 0, channel c: member 5's dx sits exactly on the lower edge of bin 7 (s = 7 exactly: a power-of-two width)
    for c in range(6):
        bins[0, 0, c] = [dx0[c] - 7 * 2.0 ** -6, 2.0 ** 6]
        assert (dx0[c] - bins[0, 0, c, 0]) * bins[0, 0, c, 1] == 7.0
    bins[0, 3, 1, 1] = 0.0                                      # inv_w = 0: everything in bin 0
    bins[0, 4, 2, 0] = np.nan                                   # NaN lo
    bins[0, 5, 6, 1] = np.nan                                   # NaN inv_w
    bins[0, 6, 0] = [np.inf, 1.0]                               # s = -inf
    bins[0, 7, 3] = [-np.inf, 1.0]                              # s = +inf: bin 63
    r = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, quantiles=Q3, bins=bins)
    assert "envelope" not in r and np.array_equal(np.stack(r["bins"]), bins, equal_nan=True)
    hist = _check(r, old, xo, uo, T, "caller's bins")
    _assert_sums(hist, np.full((1, T), B), T)
    assert hist[0, 10, 0, 0] > 0 and hist[0, 10, 0, 63] > 0 and hist[0, 10, 0, 1:63].sum() > 0   # outliers at both ends
    assert hist[0, 3, 1, 0] == B and hist[0, 4, 2, 0] == B and hist[0, 5, 6, 0] == B and hist[0, 6, 0, 0] == B
    assert hist[0, 7, 3, 63] == B
    k5 = numpy_histogram(old["xx_reg"][5:6], old["uu_reg"][5:6], xo, uo, [T], [0], bins)[0, 0, :6]
    assert np.array_equal(k5.argmax(axis=-1), np.full(6, 7))


def test_noise_and_cut_invariance():
    """192 members with the disturbance: one call against two calls (first = 0 / 128) under the same bins, merged by
    addition."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, B, seed = 200, 192, 20261016
    xo, uo, KK = _cut(g, T)
    bp = _problem(dict(g, xx_opt=xo))
    d = deltas(B)
    whole = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, sigma=SIGMA, seed=seed, quantiles=Q3)
    bins = np.stack(whole["bins"])
    run = lambda sl, first: _hist(batch.track_ensemble(bp, xo, uo, delta=d[sl], KK=KK, sigma=SIGMA, seed=seed, first=first,
                                                       quantiles=Q3, bins=bins))
    a, b = run(slice(0, 128), 0), run(slice(128, B), 128)
    assert (a.sum(axis=-1)[0, :, :6] == 128).all() and (b.sum(axis=-1)[0, :, :6] == 64).all()
    assert np.array_equal(batch.histogram_merge(a, b), _hist(whole))
    assert np.array_equal(run(slice(0, B), 0), _hist(whole))                       # and the same call again: the same counts


def test_many_tiles_per_optimum():
    """members_per_opt = 64 x 19, n_opt = 2, B = 1216 + 70, T = 40: the fold takes a full group of sixteen tiles plus three
    for optimum 0, and two tiles (one of them partial) for optimum 1."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, mpo = 40, 64 * 19
    B = mpo + 70
    XO, UO = _two_nominals(g)
    XO, UO = XO[:, :, :T], UO[:, :, :T]
    bp = _problem(dict(g, xx_opt=XO[0]))
    kw = dict(delta=deltas(B), KK=np.stack([g["KK"][:, :, :T]] * 2), members_per_opt=mpo, sigma=SIGMA, seed=11)
    r = batch.track_ensemble(bp, XO, UO, quantiles=Q3, **kw)
    old = batch.track_ensemble(bp, XO, UO, trajectories=True, **kw)
    hist = _check(r, old, XO, UO, T, "19 tiles + 2")
    _assert_sums(hist, np.stack([np.full(T, mpo), np.full(T, 70)]), T)


def test_track_ensemble_quantiles_end_to_end():
    """batch.track_ensemble(quantiles=...): with the bins of envelope['raw'] the tube is within tube_width of the order
    statistics of the returned trajectories, and every key that exists without quantiles= keeps its bits."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T, B = 200, 1000
    xo, uo, KK = _cut(g, T)
    bp = _problem(dict(g, xx_opt=xo))
    sigma = SIGMA.copy()
    sigma[2] = 1.0                                              # part of the cloud leaves: skewed, and n falls
    kw = dict(delta=deltas(B), KK=KK, sigma=sigma, seed=20261016, trajectories=True)
    qs = (0.05, 0.5, 0.95, 0.99)
    r = batch.track_ensemble(bp, xo, uo, quantiles=qs, **kw)
    old = batch.track_ensemble(bp, xo, uo, envelope=True, **kw)
    assert sorted(set(r) - set(old)) == ["bins", "hist", "quantiles", "tube", "tube_width"] and r["quantiles"] == qs
    for k in SHARED_TRAJ + ("group",):                          # (members that left carry NaN in both)
        assert np.array_equal(r[k], old[k], equal_nan=True), k
    assert r["members_per_opt"] == old["members_per_opt"] and r["summary"][0]["n_bad"] == old["summary"][0]["n_bad"] > 0
    for k, v in old["envelope"][0].items():
        assert np.array_equal(r["envelope"][0][k], v, equal_nan=True), k
    hist, bins, tube, width = r["hist"][0], r["bins"][0], r["tube"][0], r["tube_width"][0]
    assert hist.shape == (T, NCH, NBIN) and bins.shape == (T, NCH, 2) and tube.shape == (len(qs), NCH, T) and width.shape == (NCH, T)
    assert np.array_equal(bins[None], batch.histogram_bins(r["envelope"][0]["raw"]))
    t2, w2 = batch.histogram_quantiles(hist, bins, qs)
    assert np.array_equal(t2[:, 0], tube, equal_nan=True) and np.array_equal(w2[0], width)
    v = np.concatenate([r["xx_reg"] - xo, r["uu_reg"] - uo], axis=1)              # (B,8,T)
    worst = 0.0
    for t in range(T):
        live = np.flatnonzero(r["first_bad"] > t)
        for c in range(NCH if t < T - 1 else 6):
            srt = np.sort(v[live, c, t])
            for i, f in enumerate(qs):
                err = abs(tube[i, c, t] - srt[max(1, int(np.ceil(f * live.size))) - 1])
                worst = max(worst, err / width[c, t])
                assert err <= width[c, t], (f, t, c, err, width[c, t])
    assert np.isnan(tube[:, 6:, T - 1]).all()
    print("largest |tube - order statistic| / tube_width = %.3f" % worst)


def test_example_saves_the_quantiles(tmp_path):
    """examples/run_tracking_ensemble.py --quantiles FILE.npz as a process: the file's arrays equal
    batch.track_ensemble(..., quantiles=...) for the same seeded members, and the JSON line names the file."""
    import json
    from test_gpu_drivers import _run
    from aircraftoptimalcontrol_amd import batch, problems
    g, _, T = _g4()
    np.save(tmp_path / "xx_star.npy", g["xx_opt"])
    np.save(tmp_path / "uu_star.npy", g["uu_opt"])
    f = tmp_path / "tube.npz"
    out = _run("run_tracking_ensemble.py", "--data", tmp_path, "--members", 1000, "--seed", 5, "--dt", float(g["dt"]),
               "--sigma", *SIGMA, "--quantiles", f)
    line = json.loads(out.strip().split("\n")[-1])
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    d = np.random.default_rng(5).normal(size=(1000, 6)) * DELTA_SCALE
    r = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, sigma=SIGMA, seed=5, quantiles=Q3)
    saved = dict(np.load(f, allow_pickle=False))
    assert sorted(saved) == ["bins", "hist", "n", "quantiles", "tube", "tube_width"]
    assert np.array_equal(saved["quantiles"], Q3) and np.array_equal(saved["n"], r["envelope"][0]["n"])
    for k in ("bins", "hist", "tube", "tube_width"):
        assert np.array_equal(saved[k], r[k][0], equal_nan=True), k
    assert saved["hist"].shape == (T, NCH, NBIN) and saved["tube"].shape == (3, NCH, T)
    assert line["quantiles"]["file"] == str(f) and line["quantiles"]["q"] == list(Q3)
    assert np.array_equal(line["quantiles"]["max_tube_width"], np.nanmax(r["tube"][0][2, :6] - r["tube"][0][0, :6], axis=1))
    assert line["members"] == 1000 and "envelope" not in line
