"""Dense (non-diagonal) weights on every kernel family.  Every kernel is built twice, for diagonal weights and for dense
ones (the DIAG template argument, picked at run time from KConst.diag); the drivers of the reference use diagonal Q, R
and Q_T, so the dense builds are reached only here.  The weights are those of test_gpu_edges._setup(dense=True), made
exactly symmetric: the entry points that run the Riccati recursion refuse a non-symmetric Q or Q_T, and
the others must keep agreeing with the oracle for one.

  * the parity sweep of test_gpu_sweep.py (teacher-forced against the oracle, gates of check_sweep, unchanged) once per
    kernel family: the large-batch family bench.py times, the default kernels of a 4096 batch, and the knob variants
    that reach k_backward5 / k_backward4 / k_backward2, k_forward_lin, the round-based search with and without the split
    final update, and the one-wavefront forward pass with one and three candidates and the states read, not re-computed;
  * aoc_gradient, the tracking gains (k_track_gains, 2, 4; the horizon cut through aoc_mpc_step), aoc_newton_solve and
    a receding-horizon run, each with the gates of its diagonal test;
  * a non-symmetric Q: the cost, rollout and gradient entry points agree with the oracle, the Riccati ones refuse it.
Each sweep's record (dense_sweep_<name>.json) goes where test_gpu_sweep.py writes the records of its sweeps."""
import os
import time

import numpy as np
import pytest

from conftest import ROOT, rel_err
from oracle import oracle as orc
import parity_sweep
from test_gpu_sweep import LARGE_BATCH_KERNELS, check_sweep

pytestmark = pytest.mark.gpu


def _sym(M):
    return np.triu(M) + np.triu(M, 1).T


def dense_weights(Q, R, QT, seed=0, sq=1e-3, sqt=1e-2):
    """The recipe of test_gpu_edges._setup(dense=True) (and of the G14 fixtures): Q += A A^T, Q_T += A A^T, R01 = R10 =
    2e-7, each exactly symmetric whatever product NumPy picks."""
    rng = np.random.default_rng(seed)
    Q, R, QT = Q.copy(), R.copy(), QT.copy()
    for M, sc in ((Q, sq), (QT, sqt)):
        A = rng.normal(size=(6, 6)) * sc
        M += A @ A.T
    R += np.array([[0.0, 2e-7], [2e-7, 0.0]])
    Q, R, QT = _sym(Q), _sym(R), _sym(QT)
    assert all(np.array_equal(M, M.T) and np.count_nonzero(M - np.diag(np.diag(M))) == M.size - len(M) for M in (Q, R, QT))
    return Q, R, QT


def non_symmetric(Q, seed=1):
    """Q plus upper-triangle noise of 1e-3 of the diagonal scale of the dense part of the step problem's Q (~6e-6), as in
    the G14 non-symmetric case."""
    rng = np.random.default_rng(seed)
    n = Q + np.triu(rng.normal(size=(6, 6)), 1) * 1e-3 * 6e-6
    assert not np.array_equal(n, n.T)
    return n


def _step_weights():
    from aircraftoptimalcontrol_amd import problems
    pr = problems.step_maneuver(1.0, 2e-3)
    return pr, dense_weights(pr.QQt, pr.RRt, pr.QQT)


def _dump(out, name):
    """The sweep's record where test_gpu_sweep.py writes those of its sweeps, and into AOC_TEST_RECORDS."""
    from test_gpu_parity import _record
    from test_gpu_sweep import _dump as dump_sweep
    dump_sweep(out, "dense_sweep_%s.json" % name)
    _record("dense_sweep_%s.json" % name, out)


def _run_sweep(name, knobs, dist, B, n_it, tuned):
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    if knobs:
        tuned(**knobs)
    _, w = _step_weights()
    t0 = time.time()
    out = parity_sweep.sweep(aoc, problems, B, n_it, dist, "step", weights=w)
    out["tuning"] = knobs
    out["weights"] = "dense"
    out["wall_seconds"] = round(time.time() - t0, 1)
    _dump(out, name)
    check_sweep(out, B, n_it)


# (name, knobs, x0 distribution, B, iterations)
SWEEPS = [
    ("large_kernels_random", LARGE_BATCH_KERNELS, "random", 4096, 20),
    ("large_kernels_perturbed", LARGE_BATCH_KERNELS, "perturbed", 4096, 12),
    ("default_4096_random", {}, "random", 4096, 20),
    ("bw5", dict(bw_hcut=0, bw5=1), "random", 1024, 12),
    ("bw4", dict(bw_hcut=0, bw5=0), "random", 1024, 12),
    ("fw_lin", dict(fw_lin=1), "random", 1024, 12),
    ("rounds_trial_split0", dict(ls_worklist=0, nspec=2, trial_split=0), "random", 1024, 12),
    ("rounds_trial_split1", dict(ls_worklist=0, nspec=2, trial_split=1), "random", 1024, 12),
    ("one_wave_nspec1_read", dict(LARGE_BATCH_KERNELS, nspec=1, fw_recompute=0), "random", 1024, 12),
    ("one_wave_nspec3_read", dict(LARGE_BATCH_KERNELS, nspec=3, fw_recompute=0), "random", 1024, 12),
]


@pytest.mark.parametrize("name,knobs,dist,B,n_it", SWEEPS, ids=[s[0] for s in SWEEPS])
def test_dense_parity_sweep(tuned, name, knobs, dist, B, n_it):
    _run_sweep(name, knobs, dist, B, n_it, tuned)


@pytest.mark.parametrize("worklist", [0, 1])
def test_dense_gradient_vs_oracle(tuned, worklist):
    """aoc_gradient + aoc_linesearch with dense weights: the gates of test_gradient_iteration_vs_oracle_restatement, on
    the round-based search and on the work list."""
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    tuned(ls_worklist=worklist)
    pr, (Q, R, QT) = _step_weights()
    _gradient_vs_oracle(aoc, problems, pr, Q, R, QT)


def _gradient_vs_oracle(aoc, problems, pr, Q, R, QT):
    bp = aoc.BatchProblem(Q, R, QT, pr.xx_ref, pr.uu_ref, pr.dt)
    op = orc.OracleProblem(Q, R, QT, pr.xx_ref, pr.uu_ref, pr.dt)
    B = 70
    x0 = problems.perturbed_x0(pr, B, seed=3)
    prm = aoc.make_params(stepsize_0=1e-1, armijo_maxiters=20)
    oprm = orc.params(stepsize_0=1e-1, armijo_maxiters=20)
    s = aoc.GradientBatchSolver(bp, B, prm)
    s.set_initial_from_x0(x0)
    costs = []
    for kk in range(4):
        xi, ui = s.current()
        s.iterate(kk)
        sc = s.scalars()
        du = s.direction()
        xn, un = s.current()
        costs.append(sc["cost"].copy())
        assert (sc["descent"] < 0).all()
        assert np.allclose(-sc["descent"], (du ** 2).sum((1, 2)), rtol=1e-12)
        acc = sc["ntrials"] < 20
        assert (sc["cost_new"][acc] <= sc["cost"][acc] + 0.5 * sc["stepsize"][acc] * sc["descent"][acc]).all()
        for b in (0, 17, 69):
            r = orc.gradient_iterate(op, oprm, xi[b], ui[b], xi[b][:, 0])
            assert abs(r["J"] - sc["cost"][b]) <= 1e-13 * abs(r["J"])
            assert rel_err(du[b], r["du"], 1e-9) < 1e-10
            assert abs(-sc["descent"][b] - r["descent"]) <= 1e-12 * r["descent"]
            assert r["stepsize"] == sc["stepsize"][b] and r["ntrials"] == sc["ntrials"][b]
            assert rel_err(un[b], r["uu"], 1e-3) < 1e-10
            assert np.array_equal(xn[b], r["xx"]) or rel_err(xn[b], r["xx"], 1e-2) < 5e-6   # float32 flip at most
    assert (costs[-1] < costs[0]).all()


def _tracking_weights():
    from aircraftoptimalcontrol_amd import problems
    Q, R, QT = problems.tracking_weights()
    return dense_weights(Q, R, QT, seed=2, sq=1e-2, sqt=1e-2)


@pytest.mark.parametrize("knobs", [dict(track_hcut=0), dict(track_hcut=0, bw4_tiles=0), dict(track_hcut=0, split_tiles=0)],
                         ids=["k_track_gains4", "k_track_gains2", "k_track_gains"])
def test_dense_tracking_gains_vs_oracle(tuned, knobs):
    """Tracking gains and closed-loop rollout with dense tracking weights, against orc.lqr_tracking: the gates of
    test_gpu_dropin.test_tracking_batch_vs_oracle (gains 1e-8 of their scale, inputs 1e-8, states bit-identical).  The
    horizon cut of the tracking pass runs inside aoc_mpc_step (test_dense_receding_horizon)."""
    from conftest import load_golden
    from aircraftoptimalcontrol_amd import batch
    tuned(**knobs)
    g = load_golden("g4_lqr_tracking")
    T = g["xx_opt"].shape[1]
    rng = np.random.default_rng(4)
    B = 70
    XO = np.repeat(g["xx_opt"][None], B, 0); UO = np.repeat(g["uu_opt"][None], B, 0)
    UO = UO + rng.normal(0, 2.0, UO.shape)
    delta = rng.normal(0, 0.1, (B, 6))
    Q, R, QT = _tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    xr, ur, KK, st = batch.lqr_tracking_batch(bp, XO, UO, delta)
    mdl = orc.default_model(float(g["dt"]))
    for b in (0, 13, 69):
        xo, uo, Ko, ns = orc.lqr_tracking(mdl, Q, R, QT, XO[b], UO[b], delta[b])
        sc = np.abs(Ko).max(axis=-1, keepdims=True)
        assert float(np.max(np.abs(KK[b] - Ko) / np.maximum(sc, 1e-300))) < 1e-8
        assert rel_err(ur[b], uo, 1e-3) < 1e-8
        assert np.array_equal(xr[b], xo)
    assert not st.any()


@pytest.mark.parametrize("worklist", [0, 1])
@pytest.mark.parametrize("sync_every", [0, 3])
def test_dense_device_solve_equals_host_loop(tuned, sync_every, worklist):
    """aoc_newton_solve with dense weights against the host loop over aoc_newton_iterate, bit for bit (the comparison
    of test_gpu_parity.test_device_solve_equals_host_loop)."""
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    from test_gpu_parity import _same_solve
    if worklist:
        tuned(ls_worklist=1, nspec=2, split_tiles=0, split_bw_tiles=0)
    pr, (Q, R, QT) = _step_weights()
    bp = aoc.BatchProblem(Q, R, QT, pr.xx_ref, pr.uu_ref, pr.dt)
    B = 700
    x0 = problems.perturbed_x0(pr, B, seed=5)
    prm = aoc.make_params(max_iters=24, stepsize_0=1.0, armijo_maxiters=10)
    s = aoc.NewtonBatchSolver(bp, B, prm)
    s.set_initial_from_x0(x0)
    host = s.solve(compact=False)
    s.set_initial_from_x0(x0)
    dev = s.solve_on_device(sync_every=sync_every)
    assert 0 < host["converged"].sum() < B, "the case should mix stopped and unfinished trajectories"
    if sync_every == 0:
        assert dev["last_kk"] == prm.max_iters - 2
        dev["last_kk"] = host["last_kk"]
        for key in dev["history"]:
            dev["history"][key] = dev["history"][key][:, :host["history"][key].shape[1]]
    _same_solve(host, dev)


@pytest.mark.parametrize("hcut_waves", [1, 0])
def test_dense_receding_horizon(tuned, hcut_waves):
    """aoc_mpc_step with dense weights in both of its problems (the tracking pass through the horizon cut: one tile,
    T - 1 = 119 stages; hcut_waves = 1: the three-wavefront segment kernels, 0: one wavefront), against the oracle per
    instance: the loop and the gates of test_gpu_pertraj.test_receding_horizon_with_per_instance_targets."""
    from aircraftoptimalcontrol_amd import mpc, problems
    tuned(hcut_waves=hcut_waves)
    T, L = 120, 170
    full = problems.step_maneuver(tf=1.0, dt=1.0 / L)
    Q, R, QT = dense_weights(full.QQt, full.RRt, full.QQT)
    B, n_newton, n_steps, cold = 5, 2, 3, 5
    scale = np.linspace(0.6, 1.4, B)
    XR = np.repeat(full.xx_ref[None], B, 0); UR = np.repeat(full.uu_ref[None], B, 0)
    XR[:, 1] *= scale[:, None]
    pr = problems.ProblemData("mpc-dense", Q, R, QT, XR, UR, full.tt, full.tf, full.dt)
    tw = _tracking_weights()
    rh = mpc.RecedingHorizon(pr, tw, B, T, n_newton=n_newton, sigma=None, seed=7, horizon_steps=64)
    x0 = XR[:, :, 0] + np.random.default_rng(1).normal(0, 1, (B, 6)) * problems.SIGMA_X0
    rh.start(x0, cold_iters=cold)
    mdl = orc.default_model(pr.dt)
    oprm = orc.params()
    oprob = lambda b, s: orc.OracleProblem(Q, R, QT, mpc.window(XR[b], s, T), mpc.window(UR[b], s, T), pr.dt)
    XX, UU = [], []
    for b in range(B):
        xr = mpc.window(XR[b], 0, T).copy(); xr[:, 0] = x0[b]
        xx, uu = orc.initial_trajectory(mdl, xr)
        for kk in range(cold):
            r = orc.newton_iterate(oprob(b, 0), oprm, kk, xx, uu, x0[b])
            xx, uu = r["xx"], r["uu"]
        XX.append(xx); UU.append(uu)
    xg, ug = rh.solver.current()
    for b in range(B):
        assert np.array_equal(xg[b], XX[b]) and rel_err(ug[b], UU[b], 1e-3) < 1e-8
    x_true = x0.copy()
    for s in range(n_steps):
        out = rh.step()
        for b in range(B):
            op = oprob(b, s + 1)
            _, _, KK, _ = orc.lqr_tracking(mdl, tw[0], tw[1], tw[2], XX[b], UU[b], np.zeros(6))
            u_cl = UU[b][:, 0] + KK[:, :, 0] @ (x_true[b] - XX[b][:, 0])
            assert rel_err(out["u_applied"][b], u_cl, 1e-3) < 1e-8
            xn = orc.step(mdl, x_true[b], u_cl)[0]
            assert np.array_equal(out["x_true"][b], xn), (s, b)
            us = UU[b].copy(); us[:, :T - 2] = UU[b][:, 1:T - 1]
            xx, uu = orc.get_update(op, 0.0, us, np.zeros_like(us), xn)
            for kk in range(n_newton):
                r = orc.newton_iterate(op, oprm, kk, xx, uu, xn)
                xx, uu = r["xx"], r["uu"]
            XX[b], UU[b], x_true[b] = xx, uu, xn
        xg, ug = rh.solver.current()
        for b in range(B):
            assert np.array_equal(xg[b], XX[b]), (s, b)
            assert rel_err(ug[b], UU[b], 1e-3) < 1e-8, (s, b)


def test_non_symmetric_q_where_it_stays_legal():
    """A non-symmetric Q (and Q_T) on the entry points that are exact for any matrix: aoc_cost_batch (the gates of
    test_cost_batch_dense_weights), aoc_traj_cost and aoc_rollout_cost (rollouts bit-identical, costs identical to the
    last bit, as test_rollout_cost_vs_oracle) and aoc_gradient (the gates of the gradient test above)."""
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    pr, (Q, R, QT) = _step_weights()
    Qn, QTn = non_symmetric(Q, 1), non_symmetric(QT, 2)
    # unit level
    rng = np.random.default_rng(3)
    bpu = aoc.BatchProblem(Qn, R, QTn, np.zeros((6, 4)), np.zeros((2, 4)), 1e-3)
    opu = orc.OracleProblem(Qn, R, QTn, np.zeros((6, 4)), np.zeros((2, 4)), 1e-3)
    n = 100
    x, xr = rng.normal(size=(n, 6)), rng.normal(size=(n, 6))
    u, ur = rng.normal(size=(n, 2)), rng.normal(size=(n, 2))
    ll, lx, lu, llT, lTx = aoc.cost_batch(bpu, x, u, xr, ur)
    for i in range(n):
        l0, lx0, lu0 = orc.stagecost(opu, x[i], u[i], xr[i], ur[i])
        lT0, lTx0 = orc.termcost(opu, x[i], xr[i])
        assert abs(ll[i] - l0) <= 1e-13 * abs(l0) and abs(llT[i] - lT0) <= 1e-13 * abs(lT0)
        assert np.allclose(lx[i], lx0, rtol=1e-12, atol=1e-14) and np.allclose(lTx[i], lTx0, rtol=1e-12, atol=1e-14)
    # rollouts and trajectory costs
    bp = aoc.BatchProblem(Qn, R, QTn, pr.xx_ref, pr.uu_ref, pr.dt)
    op = orc.OracleProblem(Qn, R, QTn, pr.xx_ref, pr.uu_ref, pr.dt)
    B = 96
    x0 = problems.perturbed_x0(pr, B, seed=11)
    uu = np.repeat(pr.uu_ref[None], B, 0) + rng.normal(0, 1.0, (B, 2, pr.T))
    du = rng.normal(0, 1.0, (B, 2, pr.T))
    alpha = 0.7 ** rng.integers(0, 10, B)
    xx, un, J, st = aoc.rollout_cost(bp, x0, uu, du, alpha)
    Jt = aoc.traj_cost(bp, xx, un)
    for b in range(B):
        xo, uo = orc.get_update(op, alpha[b], uu[b], du[b], x0[b])
        Jo = orc.traj_cost(op, xo, uo)
        assert np.array_equal(un[b], uo) and np.array_equal(xx[b], xo), b
        assert J[b] == Jo and Jt[b] == Jo, b
    assert not st.any()
    # steepest descent
    _gradient_vs_oracle(aoc, problems, pr, Qn, R, QTn)


def test_non_symmetric_q_is_refused_by_the_riccati_entry_points():
    """aoc_newton_iterate, aoc_newton_solve, aoc_lqr_tracking, aoc_backward and the drop-in NewtonMethod raise AocError
    naming the matrix for a non-symmetric Q or Q_T, and the drop-in Cost.stagecost still evaluates it."""
    import sys
    from aircraftoptimalcontrol_amd import batch as aoc, problems, AocError
    pr, (Q, R, QT) = _step_weights()
    B = 70
    x0 = problems.perturbed_x0(pr, B, seed=3)
    prm = aoc.make_params(stepsize_0=1.0, armijo_maxiters=10)
    for Qc, QTc, name in ((non_symmetric(Q), QT, "QQt"), (Q, non_symmetric(QT), "QQT")):
        bp = aoc.BatchProblem(Qc, R, QTc, pr.xx_ref, pr.uu_ref, pr.dt)
        s = aoc.NewtonBatchSolver(bp, B, prm)
        s.set_initial_from_x0(x0)                       # (aoc_initial_trajectory accepts it)
        xi, ui = s.current()
        with pytest.raises(AocError, match="%s is not symmetric" % name):
            s.iterate(0)
        with pytest.raises(AocError, match="%s is not symmetric" % name):
            s.solve_on_device(sync_every=3)
        with pytest.raises(AocError, match="%s is not symmetric" % name):
            aoc.backward_forward(bp, xi, ui, 0)
        with pytest.raises(AocError, match="%s is not symmetric" % name):
            aoc.lqr_tracking_batch(bp, xi, ui, np.zeros(6))
    dropin = os.path.join(ROOT, "aircraftoptimalcontrol_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        import aircraft_simplified as air
        import optcon
        from conftest import load_golden
        c = load_golden("g6_chain_step_T500")
        dyn = air.Dynamics()
        dyn.dt = pr.dt
        Qn = non_symmetric(Q)
        cst = air.Cost(Qn, R, QT)
        ll, lx = cst.stagecost(c["xx_init"][:, 3], c["uu_init"][:, 3], pr.xx_ref[:, 3], pr.uu_ref[:, 3])[:2]
        op = orc.OracleProblem(Qn, R, QT, pr.xx_ref, pr.uu_ref, pr.dt)
        l0, lx0, _ = orc.stagecost(op, c["xx_init"][:, 3], c["uu_init"][:, 3], pr.xx_ref[:, 3], pr.uu_ref[:, 3])
        assert abs(float(np.squeeze(ll)) - l0) <= 1e-13 * abs(l0) and np.allclose(np.ravel(lx), lx0, rtol=1e-12, atol=1e-14)
        NM = optcon.NewtonMethod(dyn, cst, pr.xx_ref, pr.uu_ref, max_iters=5, stepsize_0=1, armijo_maxiters=10)
        with pytest.raises(AocError, match="QQt is not symmetric"):
            NM.optimize(c["xx_init"], c["uu_init"], 1.0, pr.dt)
    finally:
        sys.path.remove(dropin)
