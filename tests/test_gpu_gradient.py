"""GradientMethod.optimize (reference optcon.py:27-174) on the device.  The reference's own method raises
TypeError (armijo_stepsize called with 8 of its 9 arguments, optcon.py:125 vs :204); make_golden.py gradient runs it
with only the missing JP = JJ[kk] supplied and records every iteration (G11).  The HIP path (aoc_gradient +
aoc_linesearch) is pinned to those records (test_gradient_kernels_vs_reference), checked against the oracle's
restatement of the loop, and through the properties a steepest-descent iteration must have.  The library's Armijo
slope is -sum |du|^2 where the reference hands over +sum |du|^2."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def test_gradient_iteration_vs_oracle_restatement():
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    pr = problems.step_maneuver(1.0, 2e-3)
    bp = aoc.BatchProblem(pr.QQt, pr.RRt, pr.QQT, pr.xx_ref, pr.uu_ref, pr.dt)
    op = orc.OracleProblem(pr.QQt, pr.RRt, pr.QQT, pr.xx_ref, pr.uu_ref, pr.dt)
    B = 70
    x0 = problems.perturbed_x0(pr, B, seed=3)
    prm = aoc.make_params(stepsize_0=1e-1, armijo_maxiters=20)      # GradientMethod's own defaults are 1e-2 / 20
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
        assert (sc["descent"] < 0).all()                              # the slope: -sum |du|^2
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


def test_gradient_is_the_derivative_of_the_cost():
    """du = -dJ/du: the cost along u + eps*du falls at the rate -sum |du|^2 (finite difference through the nonlinear
    rollout; float32 state rounding limits it to a few per cent)."""
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    pr = problems.step_maneuver(1.0, 2e-3)
    bp = aoc.BatchProblem(pr.QQt, pr.RRt, pr.QQT, pr.xx_ref, pr.uu_ref, pr.dt)
    x0 = problems.perturbed_x0(pr, 64, seed=9)
    s = aoc.GradientBatchSolver(bp, 64, aoc.make_params(stepsize_0=1e-1, armijo_maxiters=20))
    s.set_initial_from_x0(x0)
    xi, ui = s.current()
    s.iterate(0)
    du, sc = s.direction(), s.scalars()
    eps = 1e-3
    _, _, J1, _ = aoc.rollout_cost(bp, x0, ui, du, np.full(64, eps), write=False)
    fd = (J1 - sc["cost"]) / eps
    assert np.allclose(fd, sc["descent"], rtol=0.05)


def test_dropin_gradient_method_runs_like_the_reference_would():
    sys.path.insert(0, os.path.join(ROOT, "aircraftoptimalcontrol_amd", "dropin"))
    import aircraft_simplified as air
    import optcon
    pg = load_golden("problem_step_T500")
    c = load_golden("g6_chain_step_T500")
    dyn = air.Dynamics(); dyn.dt = float(pg["dt"])
    GM = optcon.GradientMethod(dyn, air.Cost(pg["QQt"], pg["RRt"], pg["QQT"]), pg["xx_ref"], pg["uu_ref"], max_iters=8,
                               stepsize_0=1e-1, cc=0.5, beta=0.7, armijo_maxiters=20)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        xx_star, uu_star = GM.optimize(c["xx_init"], c["uu_init"], float(pg["tf"]), float(pg["dt"]))
    out = buf.getvalue()
    it = re.findall(r"Iter = (\d+)\t Descent = (\S+)\t Cost = (\S+)", out)
    assert out.startswith("-*-*-*-*-*-\n") and len(it) == 7 and "term =" not in out        # optcon.py:81, :143
    cost = np.array([float(v[2]) for v in it]); desc = np.array([float(v[1]) for v in it])
    assert (np.diff(cost) < 0).all() and (desc > 0).all()
    assert abs(cost[0] - c["cost"][0]) <= 1e-10 * c["cost"][0]      # the cost of the initial iterate is the Newton run's
    assert xx_star.shape == (6, 500) and uu_star.shape == (2, 500) and np.array_equal(uu_star[:, -1], uu_star[:, -2])
    # no convergence within max_iters: the last computed iterate is returned (optcon.py:137), whose cost the next
    # iteration would have printed: lower than the last printed one
    from aircraftoptimalcontrol_amd import batch as aoc
    bp = aoc.BatchProblem(pg["QQt"], pg["RRt"], pg["QQT"], pg["xx_ref"], pg["uu_ref"], float(pg["dt"]))
    us = uu_star.copy(); us[:, -1] = 0.0
    assert aoc.traj_cost(bp, xx_star[None], us[None])[0] < cost[-1]


def test_gradient_solve_stays_a_gradient_solve_when_it_compacts():
    """solve() re-packs the still-iterating trajectories into a smaller solver once fewer than half
    are active; that solver must be of the caller's class — a compacted GradientBatchSolver used to continue with
    Newton iterations.  A stopping threshold chosen so that ~60 % stop after two iterations makes the re-packing happen
    (B > compact_min); results with and without it must be identical."""
    from aircraftoptimalcontrol_amd import batch as aoc, problems
    pr = problems.step_maneuver(1.0, 2e-3)
    bp = aoc.BatchProblem(pr.QQt, pr.RRt, pr.QQT, pr.xx_ref, pr.uu_ref, pr.dt)
    B = 2200
    x0 = problems.perturbed_x0(pr, B, seed=12)
    probe = aoc.GradientBatchSolver(bp, B, aoc.make_params(stepsize_0=1e-1, armijo_maxiters=20))
    probe.set_initial_from_x0(x0)
    probe.iterate(0); probe.iterate(1)
    thr = float(np.percentile(probe.scalars()["descent"], 40))      # slopes are negative: 60 % lie above
    prm = aoc.make_params(max_iters=7, stepsize_0=1e-1, armijo_maxiters=20, term_cond=thr)
    res = []
    for compact in (True, False):
        s = aoc.GradientBatchSolver(bp, B, prm)
        s.set_initial_from_x0(x0)
        seen = []
        r = s.solve(compact=compact, callback=lambda kk, sc: seen.append(len(sc["cost"])))
        res.append((r, seen))
    (a, sa), (b, sb) = res
    assert min(sa) < B and min(sb) == B, (sa, sb)                    # the first run really re-packed
    assert a["converged"].sum() > 0.3 * B and len(set(sa)) >= 2     # some stopped early, the rest went on in a smaller batch
    for key in ("xx_star", "uu_star", "iters", "converged", "status"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for key in a["history"]:
        assert np.array_equal(a["history"][key], b["history"][key], equal_nan=True), key
    # and they are gradient iterations: every recorded slope is -sum |du|^2 < 0, after the re-packing too
    d = a["history"]["descent"]
    assert np.isfinite(d[:, -1]).any() and (d[np.isfinite(d)] < 0).all()


# ----------------------------------------------------------------------------------------------
# G11: the reference's own GradientMethod (make_golden.py gradient: JP = JJ[kk] supplied, nothing else changed)
# ----------------------------------------------------------------------------------------------
G11 = [("g11_gradient_step_T500", "problem_step_T500"), ("g11_gradient_acro_T1000", "problem_acro_T1000")]


def _g11_iterates(g, run):
    """(xx_k, uu_k) of every iteration the reference ran (as test_oracle_golden.g11_iterates): k = 0 its initial guess,
    then float32 states with sample 0 = x0 and inputs uu_{k-1} + step*deltau_{k-1}, last sample 0."""
    xx, uu = [g["xx_init"]], [g["uu_init"]]
    for k in range(len(g[run + "_JJ"]) - 1):
        x = g[run + "_xx_it"][k].astype(np.float64)
        x[:, 0] = g["xx_init"][:, 0]
        u = uu[-1] + g[run + "_stepsize"][k] * g[run + "_deltau"][k]
        u[:, -1] = 0.0
        xx.append(x); uu.append(u)
    return np.stack(xx), np.stack(uu)


def _channel_err(a, ref):
    sc = np.abs(ref).max(axis=-1, keepdims=True)
    return float(np.max(np.abs(a - ref) / np.maximum(sc, 1e-300)))


@pytest.mark.parametrize("search", ["small", "worklist"])
@pytest.mark.parametrize("run", ["def", "bt"])
@pytest.mark.parametrize("name,prob", G11)
def test_gradient_kernels_vs_reference(name, prob, run, search, tuned):
    """Every iterate k the reference's GradientMethod ran from is lane k of one batch.  aoc_gradient: J, deltau and
    +sum |deltau|^2 (= -slope) as the reference computed them.  aoc_linesearch driven through the C-ABI as
    GradientBatchSolver.iterate drives it, but handed the reference's +sum |deltau|^2: the reference's Armijo verdicts
    (step, trial count), the costs of the new iterates and their float32 states bit for bit — once with the small-batch
    search, once with the large-batch work list (split_tiles = 0, ls_worklist = 1).  A positive slope is a regime
    neither search meets otherwise.  Then the library's own slope -sum |du|^2: its verdicts equal the oracle's, and how
    many of the reference's verdicts it changes is recorded with the measured errors (AOC_TEST_RECORDS names the
    directory)."""
    import ctypes as C
    import json
    import torch
    from aircraftoptimalcontrol_amd import batch as aoc
    from aircraftoptimalcontrol_amd._lib import check, lib
    if search == "worklist":
        tuned(split_tiles=0, ls_worklist=1)
    pg = load_golden(prob)
    g = load_golden(name)
    bp = aoc.BatchProblem(pg["QQt"], pg["RRt"], pg["QQT"], pg["xx_ref"], pg["uu_ref"], float(pg["dt"]))
    op = orc.OracleProblem(pg["QQt"], pg["RRt"], pg["QQT"], pg["xx_ref"], pg["uu_ref"], float(pg["dt"]))
    kw = dict(stepsize_0=float(g[run + "_stepsize_0"]), armijo_maxiters=int(g[run + "_armijo_maxiters"]),
              cc=float(g[run + "_cc"]), beta=float(g[run + "_beta"]))
    prm, oprm = aoc.make_params(**kw), orc.params(**kw)
    XX, UU = _g11_iterates(g, run)
    n = XX.shape[0]
    J, d, st, ntr = g[run + "_JJ"], g[run + "_descent"], g[run + "_stepsize"], g[run + "_ntrials"]
    s = aoc.GradientBatchSolver(bp, n, prm)
    s.set_initial(XX, UU)
    x, f32 = s._xin()
    p = s._p(f32)
    c, nx = s.cur, (s.cur + 1) % 3
    jc, jn = s.jcur, 1 - s.jcur
    _, du, _, scratch, sbytes, _, _, _ = s._carve()
    check(lib().aoc_gradient(C.byref(p), aoc._ptr(x), aoc._ptr(s.ub[c]), aoc._ptr(s.x0), aoc._ptr(du),
                             aoc._ptr(s.descent), aoc._ptr(s.status)), "aoc_gradient")
    torch.cuda.synchronize()
    cost = s.J[jc][:n].cpu().numpy()
    slope = s.descent[:n].cpu().numpy()
    dU = s.direction()
    assert (s.status[:n] == 0).all()
    for k in range(n):
        assert abs(cost[k] - J[k]) <= 1e-12 * J[k], k
        assert _channel_err(dU[k], g[run + "_deltau"][k]) < 1e-10, k
        assert abs(-slope[k] - d[k]) <= 1e-10 * d[k], k
    status0 = s.status.clone()
    slope_dev = s.descent.clone()

    def search_with(descent):
        s.status.copy_(status0)
        s.descent.copy_(descent)
        check(lib().aoc_linesearch(C.byref(p), C.byref(prm), 0, aoc._ptr(s.ub[c]), aoc._ptr(s.x0), aoc._ptr(du),
                                   aoc._ptr(s.J[jc]), aoc._ptr(s.descent), None, aoc._ptr(s.xb[nx]), aoc._ptr(s.ub[nx]),
                                   aoc._ptr(s.J[jn]), aoc._ptr(s.stepsize), aoc._ptr(s.ntrials), aoc._ptr(s.status),
                                   aoc._ptr(scratch), sbytes, None, 0), "aoc_linesearch")
        torch.cuda.synchronize()
        xn, un = s._unpack_iterate(nx)
        return (s.stepsize[:n].cpu().numpy(), s.ntrials[:n].cpu().numpy(), s.J[jn][:n].cpu().numpy(),
                xn.cpu().numpy(), un.cpu().numpy())

    # the reference's sign
    pos = slope_dev.clone()
    pos[:n] = torch.from_numpy(d).to(pos.device)
    step, trials, cost_new, xn, un = search_with(pos)
    assert np.array_equal(step, st) and np.array_equal(trials, ntr), (step, trials, st, ntr)
    flips = 0
    for k in range(n):
        flips += int(not np.array_equal(xn[k][:, 1:].astype(np.float32), g[run + "_xx_it"][k][:, 1:]))
        if k + 1 < n:
            assert rel_err(un[k], UU[k + 1], 1e-3) < 1e-10, k
            assert abs(cost_new[k] - J[k + 1]) <= 1e-12 * J[k + 1], k
    assert flips == 0, "%d of %d new iterates differ from the reference's in a float32 state" % (flips, n)

    # the library's sign (-sum |du|^2, the slope aoc_gradient wrote): the oracle's restatement decides the same
    step_n, trials_n, _, _, _ = search_with(slope_dev)
    changed = 0
    for k in range(n):
        r = orc.gradient_iterate(op, oprm, XX[k], UU[k], XX[0][:, 0])
        assert (step_n[k], trials_n[k]) == (r["stepsize"], r["ntrials"]), k
        changed += int((step_n[k], trials_n[k]) != (st[k], ntr[k]))
    rec = dict(fixture=name, run=run, search=search, stepsize_0=kw["stepsize_0"], iterations=n, verdicts_changed=changed,
               ref_steps=st.tolist(), ref_trials=ntr.tolist(), neg_slope_steps=step_n.tolist(),
               neg_slope_trials=trials_n.tolist(), ref_cost=J.tolist(),
               max_du_err=max(_channel_err(dU[k], g[run + "_deltau"][k]) for k in range(n)),
               max_J_rel_err=float(np.max(np.abs(cost - J) / J)), max_descent_rel_err=float(np.max(np.abs(-slope - d) / d)))
    d = os.environ.get("AOC_TEST_RECORDS")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "g11_%s_%s_%s.json" % (name.split("_")[2], run, search)), "w") as f:
            json.dump(rec, f, indent=1)
