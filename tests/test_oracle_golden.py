"""The CPU oracle (oracle/aoc_oracle.c) against golden vectors captured from the reference itself
(tests/golden/make_golden.py).  Runs without a GPU.  Tolerances: unit 1e-12 rel, chains 1e-8 rel
(SURVEY 8(c)); rollouts with the reference's float32 state rounding must be bit-identical."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from oracle import oracle as orc


def _prob(name):
    g = load_golden(name)
    return g, orc.OracleProblem(g["QQt"], g["RRt"], g["QQT"], g["xx_ref"], g["uu_ref"], float(g["dt"]))


@pytest.mark.parametrize("dt", [1e-3, 2e-3])
def test_g1_step(dt):
    g = load_golden("g1_step_dt%g" % dt)
    mdl = orc.default_model(dt)
    for i in range(g["x"].shape[0]):
        xp, fx, fu, fxx, fuu, fux = orc.step(mdl, g["x"][i], g["u"][i], g["lmbd"][i])
        assert np.array_equal(xp.astype(np.float32), g["xp"][i])          # bit-exact fp32 states
        assert rel_err(fx, g["fx"][i], 1e-12) < 1e-12
        assert rel_err(fu, g["fu"][i], 1e-12) < 1e-12
        assert rel_err(fxx, g["fxx"][i], 1e-9) < 1e-12
        assert rel_err(fux, g["fux"][i], 1e-9) < 1e-12
        assert not fuu.any() and not g["fuu"][i].any()
    for i in range(g["fxx3"].shape[0]):
        r = orc.step(mdl, g["x"][i], g["u"][i], None, want3=True)
        assert rel_err(r[3], g["fxx3"][i], 1e-12) < 1e-12
        assert rel_err(r[5], g["fux3"][i], 1e-12) < 1e-12


@pytest.mark.parametrize("tag", ["step", "acro"])
def test_g2_cost(tag):
    g = load_golden("g2_cost_" + tag)
    T = 4
    p = orc.OracleProblem(g["QQt"], g["RRt"], g["QQT"], np.zeros((6, T)), np.zeros((2, T)), 1e-3)
    for i in range(g["x"].shape[0]):
        ll, lx, lu = orc.stagecost(p, g["x"][i], g["u"][i], g["xr"][i], g["ur"][i])
        assert abs(ll - g["ll"][i]) <= 1e-13 * abs(g["ll"][i])
        assert rel_err(lx, g["lx"][i], 1e-12) < 1e-13 and rel_err(lu, g["lu"][i], 1e-12) < 1e-13
        lT, lTx = orc.termcost(p, g["x"][i], g["xr"][i])
        assert abs(lT - g["llT"][i]) <= 1e-13 * abs(g["llT"][i])
        assert rel_err(lTx, g["lTx"][i], 1e-12) < 1e-13


LQR_CASES = [("a_gn_init_T1000", "problem_step_T1000"), ("b_full_init_T1000", "problem_step_T1000"),
             ("c_full_near_T500", "problem_step_T500"), ("d_gn_init_T500", "problem_step_T500")]
# Case b runs the full Hessian on the (poor) initial guess: M is indefinite at 18 stages, the
# unregularised Riccati pass (Q3) is then not contractive and amplifies last-bit differences of the
# BLAS/LAPACK summation order by ~1e3, so it is pinned at 1e-5 instead of 1e-8.
LQR_TOL = {"b_full_init_T1000": 1e-5}


def scaled_err(K, Kref):
    """max over entries of |dK| / max_t |Kref[i,j,:]| (entries of K span 8 decades)."""
    sc = np.abs(Kref).max(axis=-1, keepdims=True)
    return float(np.max(np.abs(K - Kref) / np.maximum(sc, 1e-300)))


@pytest.mark.parametrize("case,prob", LQR_CASES)
def test_g3_ltv_lqr_augmented(case, prob):
    """One backward linearisation + augmented ltv_LQR (optcon.py:429-477) incl. the regularisation
    branch (case b fires at 18 stages)."""
    g = load_golden("g3_lqr_" + case)
    _, p = _prob(prob)
    prm = orc.params()
    kk = 9 if int(g["full_hessian"]) else 0
    r = orc.newton_iterate(p, prm, kk, g["xx"], g["uu"], g["xx"][:, 0], want_internals=True)
    assert r["nreg"] == int(g["n_regularised"])
    assert r["nsing"] == 0
    KK = np.moveaxis(r["KK"], 0, -1)
    tol = LQR_TOL.get(case, 1e-8)
    assert scaled_err(KK, g["KK"]) < tol
    assert rel_err(r["du"], g["du"], 1e-3) < tol
    assert scaled_err(r["dx"], g["dx"]) < tol
    assert rel_err(r["lmbd"], g["lmbd"], 1e-9) < 1e-10
    assert abs(r["descent"] - float(g["descent"])) <= tol * abs(float(g["descent"]))


def test_g4_lqr_tracking():
    g = load_golden("g4_lqr_tracking")
    mdl = orc.default_model(float(g["dt"]))
    xr, ur, KK, ns = orc.lqr_tracking(mdl, g["QQt"], g["RRt"], g["QQT"], g["xx_opt"], g["uu_opt"], np.ones(6) * 0.1)
    assert ns == 0
    assert scaled_err(KK, g["KK"]) < 1e-8
    assert rel_err(ur, g["uu_reg"], 1e-3) < 1e-8
    # states are float32-rounded every step: exact unless a tie flips; allow no flips here
    assert np.array_equal(xr, g["xx_reg"])


CHAINS = [("g6_chain_step_T500", "problem_step_T500"), ("g6_chain_step_T1000", "problem_step_T1000"),
          ("g6_chain_acro_T1000", "problem_acro_T1000")]


@pytest.mark.parametrize("chain,prob", CHAINS)
def test_g6_chain_free_running(chain, prob):
    """N-iteration chains from the reference's initial guess: every stored iterate, every Armijo
    step and the printed Cost/Descent scalars."""
    g = load_golden(chain)
    _, p = _prob(prob)
    prm = orc.params()
    n = int(g["n_done"])
    xx, uu = g["xx_init"].copy(), g["uu_init"].copy()
    x0 = xx[:, 0].copy()
    for kk in range(n):
        r = orc.newton_iterate(p, prm, kk, xx, uu, x0)
        assert abs(r["J"] - g["cost"][kk]) <= 1e-10 * abs(g["cost"][kk]), kk
        assert abs(r["descent"] - g["descent"][kk]) <= 1e-8 * abs(g["descent"][kk]), kk
        assert r["stepsize"] == g["stepsize"][kk], kk
        assert r["ntrials"] == g["ntrials"][kk], kk
        xx, uu = r["xx"], r["uu"]
        key = "xx_it%d" % (kk + 1)
        if key in g:
            assert np.array_equal(xx, g[key]), "fp32-rounded states must match bit for bit (iter %d)" % kk
            assert rel_err(uu, g["uu_it%d" % (kk + 1)], 1e-3) < 1e-8, kk


G8 = [("g8_full_step_T500", "problem_step_T500", 22), ("g8_full_step_T1000", "problem_step_T1000", 23),
      ("g8_full_acro_T1000", "problem_acro_T1000", 37)]


def oracle_matches_g8_history(r, g):
    """How far the oracle's Armijo history equals the reference's: n if identical."""
    n = min(len(r["stepsize"]), len(g["stepsize"]))
    same = (r["stepsize"][:n] == g["stepsize"][:n]) & (r["ntrials"][:n] == g["ntrials"][:n])
    return n if same.all() and len(r["stepsize"]) == len(g["stepsize"]) else int(np.argmin(same))


@pytest.mark.parametrize("name,prob,n_ref", G8)
def test_g8_full_solve_return_index(name, prob, n_ref):
    """Full solves to the reference's own termination (configs[0]: main_newton_method.py 23 iterations at T = 1000,
    acrobatic_newton.py 37; and the T = 500 variant, 22): iteration count, returned iterate = index n_done-2 (Q7) with
    uu[:,-1] = uu[:,-2] (Q8), exhausted line searches (Q5) at the recorded iterations."""
    g = load_golden(name)
    _, p = _prob(prob)
    prm = orc.params(max_iters=200)
    r = orc.newton_optimize(p, prm, g["xx_init"], g["uu_init"])
    n = int(g["n_done"])
    assert n == n_ref
    assert (g["ntrials"] == 10).sum() >= 3          # the reference exhausts its line search several times (Q5)
    assert oracle_matches_g8_history(r, g) == n, "Armijo history leaves the reference's at iteration %d" % oracle_matches_g8_history(r, g)
    assert r["iters"] == n
    assert r["ret_index"] == n - 2
    assert np.allclose(r["cost"], g["cost"], rtol=1e-9, atol=0)
    # late iterations sit in fp32 rounding noise: descent ~1e-6 compared loosely there
    assert np.allclose(r["descent"], g["descent"], rtol=1e-6, atol=1e-9)
    assert np.array_equal(r["xx_star"], g["xx_star"])
    assert rel_err(r["uu_star"], g["uu_star"], 1e-3) < 1e-8
    assert np.array_equal(r["uu_star"][:, -1], r["uu_star"][:, -2])
    # and it is NOT the newest iterate
    assert not np.array_equal(g["xx_star"], g["xx_it%d" % n])


def test_g9_minibatch():
    g = load_golden("g9_minibatch_step_T500")
    _, p = _prob("problem_step_T500")
    prm = orc.params()
    n = int(g["n_iters"])
    xx = g["xx_init"].copy(); uu = g["uu_init"].copy()
    x0 = xx[:, :, 0].copy()
    # the P-controller initial guess itself (aircraft_simplified.py:126-148)
    mdl = orc.default_model(2e-3)
    pg = load_golden("problem_step_T500")
    for b in range(xx.shape[0]):
        xr = pg["xx_ref"].copy(); xr[:, 0] = g["x0"][b]
        xi, ui = orc.initial_trajectory(mdl, xr)
        # NOT bit-comparable: inside get_initial_trajectory the reference feeds step() its own
        # float32 output, so under NumPy-2 promotion most of that rollout is evaluated in float32
        # (outside the hot path).  The oracle evaluates in fp64 + fp32 rounding.
        assert rel_err(xi, g["xx_init"][b], 1e-2) < 2e-4 and rel_err(ui, g["uu_init"][b], 1.0) < 2e-3
    r = orc.newton_iterate_batch(p, prm, xx, uu, x0, 0, n, nthreads=4)
    assert np.array_equal(r["stepsize"], g["stepsize"])
    assert np.allclose(r["cost"], g["cost"], rtol=1e-10, atol=0)
    assert np.allclose(r["descent"], g["descent"], rtol=1e-8, atol=0)
    assert np.array_equal(xx[:, :, 1:].astype(np.float32), g["xx_out"][:, :, 1:])
    assert rel_err(uu, g["uu_out"], 1e-3) < 1e-8


def test_gradient_method_restatement_descends():
    """GradientMethod.optimize (optcon.py:27-174) restated with the missing JP argument and the slope -sum |du|^2:
    the properties of a descent method (the direction is the negative gradient, every accepted step satisfies the
    Armijo inequality, the cost decreases).  Parity with the reference: test_g11_gradient_method_teacher_forced."""
    g, p = _prob("problem_step_T500")
    c = load_golden("g6_chain_step_T500")
    prm = orc.params(stepsize_0=1e-1, armijo_maxiters=20)
    xx, uu = c["xx_init"], c["uu_init"]
    J = []
    for k in range(5):
        r = orc.gradient_iterate(p, prm, xx, uu, xx[:, 0])
        assert r["descent"] > 0 and abs(r["descent"] - (r["du"] ** 2).sum()) <= 1e-12 * r["descent"]
        xt, ut = orc.get_update(p, 1e-3, uu, r["du"], xx[:, 0])
        fd = (orc.traj_cost(p, xt, ut) - r["J"]) / 1e-3
        assert abs(fd + r["descent"]) <= 0.05 * r["descent"]
        Jn = orc.traj_cost(p, r["xx"], r["uu"])
        assert r["ntrials"] <= 20 and Jn <= r["J"] - 0.5 * r["stepsize"] * r["descent"]
        J.append(r["J"])
        xx, uu = r["xx"], r["uu"]
    assert abs(J[0] - c["cost"][0]) <= 1e-12 * J[0] and all(b < a for a, b in zip(J, J[1:]))


# ----------------------------------------------------------------------------------------------
# G11-G13 (make_golden.py gradient | ltv_general | step_wide): the surfaces the Newton chains do not reach
# ----------------------------------------------------------------------------------------------
G11 = [("g11_gradient_step_T500", "problem_step_T500"), ("g11_gradient_acro_T1000", "problem_acro_T1000")]


def g11_iterates(g, run):
    """(xx_k, uu_k) for every iteration k the reference ran: k = 0 is its initial guess; the states of k >= 1 are stored
    as float32 (sample 0 is x0), their inputs are uu_{k-1} + step*deltau_{k-1} with the last sample 0 (get_update,
    optcon.py:193-196; the generator asserts this bit for bit)."""
    xx, uu = [g["xx_init"]], [g["uu_init"]]
    for k in range(len(g[run + "_JJ"]) - 1):
        x = g[run + "_xx_it"][k].astype(np.float64)
        x[:, 0] = g["xx_init"][:, 0]
        u = uu[-1] + g[run + "_stepsize"][k] * g[run + "_deltau"][k]
        u[:, -1] = 0.0
        xx.append(x); uu.append(u)
    return xx, uu


@pytest.mark.parametrize("run", ["def", "bt"])
@pytest.mark.parametrize("name,prob", G11)
def test_g11_gradient_method_teacher_forced(name, prob, run):
    """GradientMethod.optimize of the reference, repaired only by passing JP = JJ[kk] (make_golden.py gradient), pinned
    iteration by iteration: the oracle's costate sweep from each recorded iterate gives the reference's J, deltau and
    +sum |deltau|^2; the reference's own Armijo rule (positive descent, JP = J) on the recorded deltau accepts the same
    step after the same number of trials; get_update with that step gives the next recorded iterate (float32 states
    bit for bit).  'def': constructor defaults (stepsize_0 = 1e-2, every step accepted at once); 'bt': stepsize_0 = 10,
    back-tracking with several trial counts."""
    _, p = _prob(prob)
    g = load_golden(name)
    prm = orc.params(stepsize_0=float(g[run + "_stepsize_0"]), armijo_maxiters=int(g[run + "_armijo_maxiters"]),
                     cc=float(g[run + "_cc"]), beta=float(g[run + "_beta"]))
    xs, us = g11_iterates(g, run)
    x0 = g["xx_init"][:, 0]
    n = len(g[run + "_JJ"])
    assert len(set(g[run + "_ntrials"].tolist())) >= (1 if run == "def" else 3)
    for k in range(n):
        J, dref, d = g[run + "_JJ"][k], g[run + "_deltau"][k], g[run + "_descent"][k]
        assert J == g[run + "_cost_printed"][k] and d == g[run + "_descent_printed"][k]
        r = orc.gradient_iterate(p, prm, xs[k], us[k], x0)
        assert abs(r["J"] - J) <= 1e-12 * abs(J), k
        assert scaled_err(r["du"], dref) < 1e-10, k
        assert abs(r["descent"] - d) <= 1e-10 * d, k
        s, ntr = orc.armijo(p, prm, us[k], dref, x0, d, J)
        assert (s, ntr) == (g[run + "_stepsize"][k], g[run + "_ntrials"][k]), k
        xn, un = orc.get_update(p, s, us[k], dref, x0)
        assert np.array_equal(xn[:, 1:], g[run + "_xx_it"][k][:, 1:].astype(np.float64)), k
        if k + 1 < n:
            assert rel_err(un, us[k + 1], 1e-3) < 1e-10, k
            assert abs(orc.traj_cost(p, xn, un) - g[run + "_JJ"][k + 1]) <= 1e-12 * g[run + "_JJ"][k + 1], k


def g12_case(g, case):
    """The arguments ltv_LQR was called with for one G12 case: '<case>__<arg>', else those of the case named by
    '<case>__base' (recursively) — in the reference's layout, 2-D / 1-D inputs as given (not broadcast)."""
    names = ("AA", "BB", "QQ", "RR", "SS", "QQf", "x0", "qq", "rr", "qqf")
    a, c = {}, case
    while True:
        for k in names:
            if k not in a and "%s__%s" % (c, k) in g:
                a[k] = g["%s__%s" % (c, k)]
        if "%s__base" % c not in g:
            return a
        c = str(g["%s__base" % c])


def g12_broadcast(a, T):
    """ltv_LQR's own broadcasting (optcon.py:552-651): 2-D matrices repeated over T, 1-D affine terms too."""
    b = dict(a)
    for k in ("AA", "BB", "QQ", "RR", "SS"):
        if b[k].ndim == 2:
            b[k] = np.repeat(b[k][:, :, None], T, axis=2)
    for k in ("qq", "rr"):
        if k in b and b[k].ndim == 1:
            b[k] = np.repeat(b[k][:, None], T, axis=1)
    return b


G12_CASES = ["plain0", "aug0", "plain1", "aug1", "ti_plain", "ti_aug", "short2", "short3", "indef", "indef_aug", "complex"]


def test_g12_case_list():
    assert [str(c) for c in load_golden("g12_ltv_general")["cases"]] == G12_CASES


@pytest.mark.parametrize("case", G12_CASES)
def test_g12_ltv_lqr_general(case):
    """optcon.ltv_LQR on problems the aircraft never produces (make_golden.py ltv_general): dense R, S != 0, x0 != 0,
    affine terms, broadcast 2-D / 1-D inputs, T = 2 and 3, indefinite and non-symmetric R.  KK, PP, xx, uu within 1e-10
    of each entry's scale over t (1e-8 where the gain loop regularises) and the same number of regularised stages."""
    g = load_golden("g12_ltv_general")
    T = int(g[case + "__TT"])
    a = g12_broadcast(g12_case(g, case), T)
    KK, PP, xx, uu, nreg, ns = orc.ltv_lqr(a["AA"], a["BB"], a["QQ"], a["RR"], a["SS"], a["QQf"], a["x0"],
                                           a.get("qq"), a.get("rr"), a.get("qqf"))
    assert ns == 0
    assert nreg == int(g[case + "__n_regularised"])
    tol = 1e-8 if nreg else 1e-10
    for got, key in ((KK, "KK"), (PP, "PP"), (xx, "xx"), (uu, "uu")):
        ref = g["%s__%s" % (case, key)]
        assert got.shape == ref.shape, key
        assert scaled_err(got, ref) < tol, (key, scaled_err(got, ref))


def test_g13_step_wide():
    """Dynamics.step beyond G1's box (make_golden.py step_wide): angles over +-4 pi with points 1e-9 either side of
    every k pi/4, angles in [2^20, 2^24], V from 0.05 to 300.  Gates of test_g1_step."""
    g = load_golden("g13_step_wide")
    mdl = orc.default_model(float(g["dt"]))
    for i in range(g["x"].shape[0]):
        xp, fx, fu, fxx, fuu, fux = orc.step(mdl, g["x"][i], g["u"][i], g["lmbd"][i])
        assert np.array_equal(xp.astype(np.float32), g["xp"][i]), i
        assert rel_err(fx, g["fx"][i], 1e-12) < 1e-12, i
        assert rel_err(fu, g["fu"][i], 1e-12) < 1e-12, i
        assert rel_err(fxx, g["fxx"][i], 1e-9) < 1e-12, i
        assert rel_err(fux, g["fux"][i], 1e-9) < 1e-12, i
        assert not fuu.any() and not g["fuu"][i].any()
    for j, i in enumerate(g["sel3"]):
        r = orc.step(mdl, g["x"][i], g["u"][i], None, want3=True)
        assert rel_err(r[3], g["fxx3"][j], 1e-12) < 1e-12
        assert rel_err(r[5], g["fux3"][j], 1e-12) < 1e-12


G14_CHAINS = ["g14_dense_step_T500", "g14_dense_nonsym_q_step_T500"]


@pytest.mark.parametrize("chain", G14_CHAINS)
def test_g14_dense_weights_chain_teacher_forced(chain):
    """NewtonMethod with dense weights (make_golden.py dense): dense symmetric Q, R, Q_T, and the same with a
    non-symmetric Q, on the step problem at T = 500, 11 iterations from the reference's initial guess (full Hessian from
    kk = 9).  Each iteration is redone by the oracle from the reference's own iterate; the gates of
    test_g6_chain_free_running: every Armijo step and trial count identical, cost within 1e-10 and descent within 1e-8,
    states bit-identical and inputs within 1e-8 of their scale."""
    g = load_golden(chain)
    pr = load_golden("problem_step_T500")
    p = orc.OracleProblem(g["QQt"], g["RRt"], g["QQT"], pr["xx_ref"], pr["uu_ref"], float(pr["dt"]))
    assert np.array_equal(g["QQT"], g["QQT"].T) and np.array_equal(g["RRt"], g["RRt"].T)
    assert np.array_equal(g["QQt"], g["QQt"].T) == (chain == "g14_dense_step_T500")
    assert np.count_nonzero(g["QQt"] - np.diag(np.diag(g["QQt"]))) == 30      # dense
    prm = orc.params()
    n = int(g["n_done"])
    assert n == 11 and len(g["stepsize"]) == n
    xx, uu = g["xx_init"], g["uu_init"]
    x0 = xx[:, 0].copy()
    for kk in range(n):
        r = orc.newton_iterate(p, prm, kk, xx, uu, x0)
        assert abs(r["J"] - g["cost"][kk]) <= 1e-10 * abs(g["cost"][kk]), kk
        assert abs(r["descent"] - g["descent"][kk]) <= 1e-8 * abs(g["descent"][kk]), kk
        assert r["stepsize"] == g["stepsize"][kk] and r["ntrials"] == g["ntrials"][kk], kk
        xx, uu = g["xx_it%d" % (kk + 1)], g["uu_it%d" % (kk + 1)]
        assert np.array_equal(r["xx"], xx), "fp32-rounded states must match bit for bit (iter %d)" % kk
        assert rel_err(r["uu"], uu, 1e-3) < 1e-8, kk


def test_g14_ltv_lqr_non_symmetric_q():
    """The generic ltv_LQR with a non-symmetric Q_t at every stage and a non-symmetric Qf (make_golden.py dense): the
    gates of test_g12_ltv_lqr_general."""
    g = load_golden("g14_ltv_nonsym")
    assert not np.array_equal(g["QQf"], g["QQf"].T)
    KK, PP, xx, uu, nreg, ns = orc.ltv_lqr(g["AA"], g["BB"], g["QQ"], g["RR"], g["SS"], g["QQf"], g["x0"], g["qq"], g["rr"],
                                           g["qqf"])
    assert ns == 0
    assert nreg == int(g["n_regularised"])
    tol = 1e-8 if nreg else 1e-10
    for got, key in ((KK, "KK"), (PP, "PP"), (xx, "xx"), (uu, "uu")):
        assert got.shape == g[key].shape, key
        assert scaled_err(got, g[key]) < tol, (key, scaled_err(got, g[key]))
