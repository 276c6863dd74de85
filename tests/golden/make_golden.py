#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING the reference.

This script only works in the build container, where the upstream repository is
mounted read-only at /root/reference.  It imports the reference's three library
modules (optcon, aircraft_simplified, lqr_tracking) headlessly, drives them with
the parameters of the reference's own driver scripts, and saves inputs + outputs
as small .npz fixtures.  Nothing of the reference travels: fixtures hold numbers
only.  The driver scripts themselves are NOT imported (they need cvxpy and call
plt.show/np.save at import); the problem set-up they do is re-stated below from
main_newton_method.py:32-142 and acrobatic_newton.py:34-154.

Run:  MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden.py [SUBCOMMAND]

Without a subcommand the fixtures g1-g10, problem_* and data_* are written.  A subcommand writes only its own:
  config1      g8_full_{step,acro}_T1000          the drivers' full solves at T = 1000
  airfoil      g10_airfoil                        animate.Airfoil outlines and frames
  gradient     g11_gradient_{step_T500,acro_T1000}  GradientMethod.optimize with the missing JP supplied, every
                                                  iteration (defaults, and stepsize_0 = 10 to back-track)
  ltv_general  g12_ltv_general                    the generic ltv_LQR on seeded random problems (dense R, S, affine
                                                  and broadcast inputs, T = 2 / 3, indefinite and non-symmetric R)
  step_wide    g13_step_wide                      Dynamics.step at angles over +-4 pi, 1e-9 from every k pi/4, in
                                                  [2^20, 2^24], and V from 0.05 to 300
  dense        g14_dense_step_T500, g14_dense_nonsym_q_step_T500, g14_ltv_nonsym
                                                  NewtonMethod with dense symmetric weights and with a non-symmetric Q
                                                  (11 iterations, every iterate), ltv_LQR with non-symmetric Q and Qf
"""
import contextlib
import io
import os
import re
import sys
import warnings

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REF = "/root/reference"
sys.path.insert(0, REF)
warnings.simplefilter("ignore")

import aircraft_simplified as ref_air  # noqa: E402
import lqr_tracking as ref_lqr  # noqa: E402
import optcon as ref_opt  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print("wrote %-28s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


# --------------------------------------------------------------------------------------
# problem set-up (parameters of the reference's drivers)
# --------------------------------------------------------------------------------------
def sigmoid(tt, slope):
    ss = 1 / (1 + np.exp((-tt) * slope))
    return ss, ss * (1 - ss)


def step_problem(tf=1.0, dt=1e-3):
    """main_newton_method.py:50-142 (weights, sigmoid reference, equilibrium input)."""
    dyn = ref_air.Dynamics()
    ns, ni = dyn.ns, dyn.ni
    QQt = np.eye(ns) * 1e-6
    QQt[1, 1] = dyn.m * dyn.g * 0.01
    QQt[2, 2] = 0.5 * dyn.m * 0.001
    QQt[3, 3] = 0.01
    QQt[4, 4] = 0.5 * dyn.J * 0.001
    RRt = 1e-6 * np.eye(ni)
    QQT = QQt.copy()
    QQT[1, 1] = QQT[1, 1] * 20
    QQT[3, 3] = QQT[1, 1]
    QQT[0, 0] = QQT[1, 1]
    dyn.dt = dt
    TT = int(tf / dt)
    tt = np.linspace(0, tf, TT)
    x0, z0, xf, zf = 0, 0, 16, 2.71
    slope = tt.shape[0] * 1
    zz = z0 + sigmoid(tt - tt[-1] / 2, slope)[0] * (zf - z0)
    zzd = sigmoid(tt - tt[-1] / 2, slope)[1] * (zf - z0)
    xxe, uue = dyn.get_equilibrium(np.zeros(ns,), tt)
    xx_ref = np.zeros((ns, TT))
    uu_ref = np.zeros((ni, TT))
    xx_ref[0, :] = x0 + ((xf - x0) / tf) * tt
    xx_ref[1, :] = zz
    xx_ref[2, :] = (zzd ** 2 + ((xf - x0) / tf) ** 2) ** 0.5
    for i in range(ni):
        uu_ref[i, :] = uue[i]
    return dict(dyn=dyn, QQt=QQt, RRt=RRt, QQT=QQT, xx_ref=xx_ref, uu_ref=uu_ref,
                tt=tt, tf=tf, dt=dt, TT=TT, xxe=np.asarray(xxe, float), uue=np.asarray(uue))


def acro_problem(tf=1.0, dt=1e-3):
    """acrobatic_newton.py:52-154."""
    dyn = ref_air.Dynamics()
    ns, ni = dyn.ns, dyn.ni
    QQt = np.eye(ns) * 1e-6
    QQt[1, 1] = dyn.m * dyn.g * 0.01
    QQt[2, 2] = 0.5 * dyn.m * 0.001
    QQt[3, 3] = 0.01
    QQt[4, 4] = 0.5 * dyn.J * 0.001
    RRt = 1e-6 * np.eye(ni)
    QQT = QQt.copy()
    QQT[1, 1] = QQT[1, 1] * 100
    QQT[3, 3] = QQT[1, 1]
    QQT[0, 0] = QQT[1, 1]
    dyn.dt = dt
    TT = int(tf / dt)
    tt = np.linspace(0, tf, TT)
    x0, z0, xf, zf = 0, 0, 18, 2.71
    slope = tt.shape[0] * 0.1
    pp = np.zeros((TT,))
    pp[:TT // 2] = z0 + sigmoid(tt[:TT // 2] - tt[TT // 2] / 2, slope)[0] * (zf - z0)
    pp[TT // 2:] = z0 + sigmoid(-tt[:TT // 2] + tt[TT // 2] / 2, slope)[0] * (zf - z0)
    temp = pp.copy()
    N = pp.shape[0]
    pp = np.zeros(temp.shape)
    pp[int(0.05 * N):int(0.50 * N)] = temp[:int(0.45 * N)]
    pp[int(0.50 * N):int(0.95 * N)] = temp[-int(0.45 * N):]
    xxe, uue = dyn.get_equilibrium(np.zeros(ns,), tt)
    xx_ref = np.zeros((ns, TT))
    uu_ref = np.zeros((ni, TT))
    xx_ref[0, :] = x0 + ((xf - x0) / tf) * tt
    xx_ref[1, :] = pp
    for i in range(2, ns):
        xx_ref[i, :] = xxe[i]
    xx_ref[3, :] = 0.0
    for i in range(ni):
        uu_ref[i, :] = uue[i]
    uu_ref[0, :] = uu_ref[0, :] * 10
    uu_ref[1, :] = -60
    return dict(dyn=dyn, QQt=QQt, RRt=RRt, QQT=QQT, xx_ref=xx_ref, uu_ref=uu_ref,
                tt=tt, tf=tf, dt=dt, TT=TT, xxe=np.asarray(xxe, float), uue=np.asarray(uue))


def problem_arrays(p):
    return dict(QQt=p["QQt"], RRt=p["RRt"], QQT=p["QQT"], xx_ref=p["xx_ref"], uu_ref=p["uu_ref"],
                dt=np.float64(p["dt"]), tf=np.float64(p["tf"]), TT=np.int64(p["TT"]))


# --------------------------------------------------------------------------------------
# running the reference optimiser with taps on its own methods
# --------------------------------------------------------------------------------------
ITER_RE = re.compile(r"Iter = (\d+)\t Descent = (\S+)\t Cost = (\S+)")


def run_newton(p, xx_init, uu_init, n_iters, keep, armijo_maxiters=10, stepsize_0=1, cc=0.5, beta=0.7):
    """Run NewtonMethod(max_iters=n_iters+1).optimize; record every iterate the reference
    produces (return values of its get_update), the Armijo step sizes and the stdout scalars."""
    cst = ref_air.Cost(p["QQt"], p["RRt"], p["QQT"])
    NM = ref_opt.NewtonMethod(p["dyn"], cst, p["xx_ref"], p["uu_ref"], max_iters=n_iters + 1,
                              stepsize_0=stepsize_0, cc=cc, beta=beta,
                              armijo_maxiters=armijo_maxiters, term_cond=1e-6, visu_armijo=False)
    iterates, steps, ntrials = [], [], []
    orig_update, orig_armijo = NM.get_update, NM.armijo_stepsize
    ncalls = {"n": 0}
    dyn = p["dyn"]
    orig_step = dyn.step

    def tap_step(*a):
        ncalls["n"] += 1
        return orig_step(*a)

    def tap_update(stepsize, uu, deltau, x0):
        xx_t, uu_t = orig_update(stepsize, uu, deltau, x0)
        iterates.append((xx_t.copy(), uu_t.copy()))
        return xx_t, uu_t

    def tap_armijo(*a):
        n0 = ncalls["n"]
        s = orig_armijo(*a)
        ntrials.append((ncalls["n"] - n0) // (p["TT"] - 1))
        steps.append(float(s))
        return s

    NM.get_update, NM.armijo_stepsize, dyn.step = tap_update, tap_armijo, tap_step
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            xx_star, uu_star = NM.optimize(xx_init.copy(), uu_init.copy(), p["tf"], p["dt"])
    finally:
        dyn.step = orig_step
    xx_star, uu_star = xx_star.copy(), uu_star.copy()
    txt = buf.getvalue()
    sc = [(int(a), float(b), float(c)) for a, b, c in ITER_RE.findall(txt)]
    out = dict(descent=np.array([s[1] for s in sc]), cost=np.array([s[2] for s in sc]),
               stepsize=np.array(steps), ntrials=np.array(ntrials, dtype=np.int64),
               xx_star=xx_star, uu_star=uu_star, n_done=np.int64(len(sc)),
               xx_init=xx_init, uu_init=uu_init)
    for k in keep:
        if 1 <= k <= len(iterates):
            out["xx_it%d" % k] = iterates[k - 1][0]
            out["uu_it%d" % k] = iterates[k - 1][1]
    return out, iterates


def backward_quantities(p, xx, uu, full_hessian):
    """The linearisation loop of optcon.py:429-464, executed with the reference's own functions."""
    dyn = p["dyn"]
    cst = ref_air.Cost(p["QQt"], p["RRt"], p["QQT"])
    ns, ni, TT = 6, 2, p["TT"]
    xr, ur = p["xx_ref"], p["uu_ref"]
    QQ = np.zeros((ns, ns, TT)); RR = np.zeros((ni, ni, TT)); SS = np.zeros((ni, ns, TT))
    qq = np.zeros((ns, TT)); rr = np.zeros((ni, TT))
    AA = np.zeros((ns, ns, TT)); BB = np.zeros((ns, ni, TT)); lmbd = np.zeros((ns, TT))
    lT, QT = cst.termcost(xx[:, TT - 1], xr[:, TT - 1])[1:]
    lmbd[:, TT - 1] = lT.squeeze(); QQ[:, :, TT - 1] = QT; qq[:, TT - 1] = lT.squeeze()
    for t in reversed(range(TT - 1)):
        aa, bb, lxx, lxu, lux, luu = cst.stagecost(xx[:, t], uu[:, t], xr[:, t], ur[:, t])[1:]
        fx, fu, fxx, fuu, fux = dyn.step(xx[:, t], uu[:, t], lmbd[:, t + 1])[1:]
        A, Bm = fx.T, fu.T
        if full_hessian:
            QQ[:, :, t] = lxx + fxx; RR[:, :, t] = luu + fuu; SS[:, :, t] = lux + fux
        else:
            QQ[:, :, t] = lxx; RR[:, :, t] = luu; SS[:, :, t] = lux
        AA[:, :, t] = A; BB[:, :, t] = Bm; qq[:, t] = aa.squeeze(); rr[:, t] = bb.squeeze()
        lmbd[:, t] = (A.T @ lmbd[:, t + 1][:, None] + aa).squeeze()
    return AA, BB, QQ, RR, SS, qq, rr, lmbd


def lqr_case(p, xx, uu, full_hessian):
    AA, BB, QQ, RR, SS, qq, rr, lmbd = backward_quantities(p, xx, uu, full_hessian)
    TT = p["TT"]
    nreg = {"n": 0}
    orig = np.linalg.eigvals

    def tap(M):
        w = orig(M)
        if not np.all(w > 0):
            nreg["n"] += 1
        return w

    np.linalg.eigvals = tap
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            KK, PP, dx, du = ref_opt.ltv_LQR(AA, BB, QQ, RR, SS, QQ[:, :, TT - 1], TT, np.zeros(6),
                                             qq, rr, qq[:, TT - 1])
    finally:
        np.linalg.eigvals = orig
    descent = 0.0
    for t in reversed(range(TT - 1)):
        descent += float(((BB[:, :, t].T @ lmbd[:, t + 1][:, None] + rr[:, t][:, None]).T
                          @ du[:, t].reshape((2, 1))).item())
    return dict(xx=xx, uu=uu, full_hessian=np.int64(full_hessian), KK=KK, PP_s=PP[:, :, ::50].copy(),
                dx=dx.copy(), du=du.copy(), lmbd=lmbd, descent=np.float64(descent),
                n_regularised=np.int64(nreg["n"]))


def full_solve(p, name):
    """G8: NewtonMethod(max_iters=200).optimize to its own termination — iteration count, Armijo steps and trial
    counts, stdout scalars, the returned iterate (index n_done-2, Q7) and its neighbours."""
    xi, ui = p["dyn"].get_initial_trajectory(p["xx_ref"], p["tt"])
    full, its = run_newton(p, xi, ui, 199, ())
    nd = int(full["n_done"])
    for k in (nd - 2, nd - 1, nd):
        if 1 <= k <= len(its):
            full["xx_it%d" % k], full["uu_it%d" % k] = its[k - 1]
    save(name, **full)
    print("full solve %s: iterations printed = %d, cost %r -> %r, ntrials %s" %
          (name, nd, float(full["cost"][0]), float(full["cost"][-1]), full["ntrials"].tolist()))


def config1_full_solves():
    """BASELINE configs[0] / SURVEY 8d config 1: the two drivers of the reference at their native T = 1000
    (main_newton_method.py:32-142: 23 iterations, returned iterate 21; acrobatic_newton.py:34-154: 37 iterations)."""
    full_solve(step_problem(), "g8_full_step_T1000")
    full_solve(acro_problem(), "g8_full_acro_T1000")


def airfoil_vectors():
    """the post-processing module animate.py (:6-140).  The outline of Airfoil(20, ...) (the thickness both
    drivers use, main_newton_method.py:226, acrobatic_newton.py:242) and of a 12 % section, the outline at seeded random
    poses through update_pose, and what animate(i) puts into its artists for a few frames of a seeded trajectory (the
    artists are made here, as run_animation makes them, without rendering 1000 frames)."""
    import matplotlib.pyplot as plt
    import animate as ref_anim
    rng = np.random.default_rng(20261005)
    dt, TT = 0.05, 20
    xs = np.stack([np.linspace(0, 16, TT), 3 * np.sin(np.linspace(0, 3, TT)), rng.uniform(9, 23, TT),
                   rng.uniform(-3.2, 3.2, TT), rng.normal(0, 5, TT), rng.uniform(-1, 1, TT)])
    xr = xs + rng.normal(0, 0.3, xs.shape)
    af = ref_anim.Airfoil(20, xs, xr, dt=dt, xlim=[0, 17], ylim=[-5, 5])
    outline20 = af.update_pose(0.0, 0.0, 0.0)            # T = identity
    outline12 = ref_anim.Airfoil(12, xs, xr).update_pose(0.0, 0.0, 0.0)
    n = 16
    th, px, py = rng.uniform(-3.2, 3.2, n), rng.uniform(-2, 20, n), rng.uniform(-5, 5, n)
    posed = np.stack([af.update_pose(th[i], px[i], py[i]) for i in range(n)])
    fig, ax = plt.subplots()
    af.line0, = ax.plot([], []); af.line1, = ax.plot([], []); af.point1, = ax.plot([], [])
    af.time_template = 't = %.1f s'; af.time_text = ax.text(0, 0, '')
    frames = np.array([0, 7, 19])
    l0 = []; l1 = []
    point_error = ""
    for i in frames:
        try:
            af.animate(int(i))
        except RuntimeError as e:        # Matplotlib >= 3.7 refuses the scalars animate.py:111 hands to point1.set_data:
            point_error = str(e)         # the two outlines are set by then, the marker and the time label are not
        l0.append(np.stack(af.line0.get_data())); l1.append(np.stack(af.line1.get_data()))
    plt.close(fig)
    save("g10_airfoil", xx_star=xs, xx_ref=xr, dt=np.float64(dt), outline20=outline20, outline12=outline12,
         theta=th, x_loc=px, y_loc=py, posed=posed, frames=frames, line0=np.stack(l0), line1=np.stack(l1),
         point_error=np.array(point_error))


class _GradientMethodJP(ref_opt.GradientMethod):
    """The reference's GradientMethod with the one repair that lets optimize() run: armijo_stepsize is called with 8 of
    its 9 arguments (optcon.py:125 vs :204); the missing JP is the cost JJ[kk] the caller already passes.  The loop of
    optcon.py:84-148 and the +sum |du|^2 it hands over as `descent` are the reference's own."""

    def armijo_stepsize(self, uu, deltau, xx_ref, uu_ref, x0, TT, JJ, descent, JP=None):
        return super().armijo_stepsize(uu, deltau, xx_ref, uu_ref, x0, TT, JJ, descent, JJ)


def next_inputs(uu, stepsize, deltau):
    """The inputs get_update makes (optcon.py:193-196): uu + stepsize*deltau, the last sample 0."""
    un = uu + stepsize * deltau
    un[:, -1] = 0.0
    return un


def run_gradient(p, xx_init, uu_init, n_iters, stepsize_0=1e-2, armijo_maxiters=20, cc=0.5, beta=0.7):
    """GradientMethod(max_iters=n_iters+1).optimize with taps on get_update / armijo_stepsize (as run_newton): per
    iteration k the iterate k it started from, JJ[k], descent[k] and deltau as handed to Armijo, the accepted step, the
    trial count and the stdout scalars.  States of iterates k >= 1 are float32 values past sample 0 (stored so)."""
    cst = ref_air.Cost(p["QQt"], p["RRt"], p["QQT"])
    GM = _GradientMethodJP(p["dyn"], cst, p["xx_ref"], p["uu_ref"], max_iters=n_iters + 1, stepsize_0=stepsize_0,
                           cc=cc, beta=beta, armijo_maxiters=armijo_maxiters, visu_armijo=False)
    iterates, armijo_in, steps, ntrials = [], [], [], []
    orig_update, orig_armijo = GM.get_update, GM.armijo_stepsize
    ncalls = {"n": 0}
    dyn = p["dyn"]
    orig_step = dyn.step

    def tap_step(*a):
        ncalls["n"] += 1
        return orig_step(*a)

    def tap_update(stepsize, uu, deltau, x0):
        xx_t, uu_t = orig_update(stepsize, uu, deltau, x0)
        iterates.append((xx_t.copy(), uu_t.copy()))
        return xx_t, uu_t

    def tap_armijo(uu, deltau, xx_ref, uu_ref, x0, TT, JJ, descent):
        armijo_in.append((uu.copy(), deltau.copy(), float(JJ), float(descent)))
        n0 = ncalls["n"]
        s = orig_armijo(uu, deltau, xx_ref, uu_ref, x0, TT, JJ, descent)
        ntrials.append((ncalls["n"] - n0) // (p["TT"] - 1))
        steps.append(float(s))
        return s

    GM.get_update, GM.armijo_stepsize, dyn.step = tap_update, tap_armijo, tap_step
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            GM.optimize(xx_init.copy(), uu_init.copy(), p["tf"], p["dt"])
    finally:
        dyn.step = orig_step
    import matplotlib.pyplot as plt
    plt.close("all")
    sc = [(int(a), float(b), float(c)) for a, b, c in ITER_RE.findall(buf.getvalue())]
    n = len(sc)
    assert n == n_iters == len(steps) == len(iterates) and [s[0] for s in sc] == list(range(n))
    J = np.array([a[2] for a in armijo_in]); d = np.array([a[3] for a in armijo_in])
    assert np.array_equal(J, [s[2] for s in sc]) and np.array_equal(d, [s[1] for s in sc])
    # what Armijo was handed at iteration k is iterate k; iterate k+1 is what get_update made of it
    assert np.array_equal(armijo_in[0][0], uu_init)
    for k in range(1, n):
        assert np.array_equal(armijo_in[k][0], iterates[k - 1][1])
    xx_it = np.stack([it[0] for it in iterates])
    assert np.array_equal(xx_it[:, :, 1:].astype(np.float32), xx_it[:, :, 1:])
    assert (xx_it[:, :, 0] == xx_init[:, 0]).all()
    # the inputs of iterate k+1 are not stored: they are uu_k + step_k*deltau_k (last sample 0), bit for bit
    for k in range(n):
        assert np.array_equal(iterates[k][1], next_inputs(armijo_in[k][0], steps[k], armijo_in[k][1]))
    return dict(xx_init=xx_init, uu_init=uu_init, JJ=J, descent=d,
                deltau=np.stack([a[1] for a in armijo_in]), stepsize=np.array(steps),
                ntrials=np.array(ntrials, dtype=np.int64), xx_it=xx_it.astype(np.float32),
                cost_printed=np.array([s[2] for s in sc]),
                descent_printed=np.array([s[1] for s in sc]), stepsize_0=np.float64(stepsize_0),
                armijo_maxiters=np.int64(armijo_maxiters), cc=np.float64(cc), beta=np.float64(beta))


def gradient_vectors():
    """G11: GradientMethod.optimize (optcon.py:27-174) with JP supplied, from the reference's own initial guess
    (the xx_init / uu_init of g6_*): the constructor defaults (stepsize_0 = 1e-2, armijo_maxiters = 20: every step is
    accepted at its first trial) and stepsize_0 = 10 (back-tracking; the reference's +sum |du|^2 slope then accepts
    steps that raise the cost).  Keys 'def_*' and 'bt_*'; xx_it[k] holds the states of iterate k+1, whose inputs are
    next_inputs(inputs of iterate k, stepsize[k], deltau[k])."""
    for name, p, n_iters in (("g11_gradient_step_T500", step_problem(tf=1.0, dt=2e-3), 7),
                             ("g11_gradient_acro_T1000", acro_problem(), 3)):
        xi, ui = p["dyn"].get_initial_trajectory(p["xx_ref"], p["tt"])
        out = {}
        for tag, s0 in (("def", 1e-2), ("bt", 10.0)):
            r = run_gradient(p, xi, ui, n_iters, stepsize_0=s0)
            if tag == "def":
                assert (r["ntrials"] == 1).all()
            else:
                assert len(set(r["ntrials"].tolist())) >= 3, r["ntrials"]
            print("  G11 %s %s: steps %s, trials %s, cost %r -> %r" % (name, tag, r["stepsize"].tolist(),
                  r["ntrials"].tolist(), float(r["JJ"][0]), float(r["JJ"][-1])))
            for k, v in r.items():
                if k not in ("xx_init", "uu_init"):
                    out[tag + "_" + k] = v
        save(name, xx_init=xi, uu_init=ui, **out)


def ltv_general_vectors():
    """G12: the generic optcon.ltv_LQR (optcon.py:533-771) on seeded random problems the aircraft never produces:
    dense per-stage A, B, Q, R (SPD, non-diagonal), S != 0, x0 != 0; the same augmented with per-stage qq / rr and a
    qqf; time-invariant 2-D inputs with 1-D affine terms (the reference repeats them); T = 2 and T = 3; an R_t with a
    negative eigenvalue at some stages (the gain loop regularises, the Riccati loop does not); a non-symmetric R that
    gives M complex eigenvalues with positive and negative real parts.  Per case '<case>__<arg>' holds what ltv_LQR was
    called with ('<case>__base' names the case whose arrays it shares, to keep the file small) and KK, PP, xx, uu and
    the number of regularised stages (an eigvals tap, as lqr_case)."""
    rng = np.random.default_rng(20261016)

    def spd(n, lo, hi):
        Qm, _ = np.linalg.qr(rng.normal(size=(n, n)))
        return Qm @ np.diag(rng.uniform(lo, hi, n)) @ Qm.T

    def stage_set(T):
        A = np.stack([0.9 * np.linalg.qr(rng.normal(size=(6, 6)))[0] + 0.08 * rng.normal(size=(6, 6)) for _ in range(T)], -1)
        return dict(AA=A, BB=0.3 * rng.normal(size=(6, 2, T)), QQ=np.stack([spd(6, 0.1, 2.0) for _ in range(T)], -1),
                    RR=np.stack([spd(2, 0.05, 1.0) for _ in range(T)], -1), SS=0.05 * rng.normal(size=(2, 6, T)),
                    QQf=spd(6, 0.5, 5.0), x0=rng.normal(0, 1, 6))

    def affine(T):
        return dict(qq=rng.normal(0, 1, (6, T)), rr=rng.normal(0, 1, (2, T)), qqf=rng.normal(0, 1, 6))

    T = 40
    cases = {}
    for i in (0, 1):
        cases["plain%d" % i] = stage_set(T)
        cases["aug%d" % i] = dict(base="plain%d" % i, **affine(T))
    ti = dict(AA=0.9 * np.linalg.qr(rng.normal(size=(6, 6)))[0] + 0.08 * rng.normal(size=(6, 6)),
              BB=0.3 * rng.normal(size=(6, 2)), QQ=spd(6, 0.1, 2.0), RR=spd(2, 0.05, 1.0), SS=0.05 * rng.normal(size=(2, 6)),
              QQf=spd(6, 0.5, 5.0), x0=rng.normal(0, 1, 6))
    cases["ti_plain"] = dict(TT=T, **ti)
    cases["ti_aug"] = dict(base="ti_plain", qq=rng.normal(0, 1, 6), rr=rng.normal(0, 1, 2), qqf=rng.normal(0, 1, 6))
    cases["short2"] = dict(**stage_set(2), **affine(2))
    cases["short3"] = stage_set(3)
    # R_t indefinite at every fifth stage: eigenvalues (-1, 0.5) — M = R + B^T P B keeps a negative one
    Rneg = cases["plain0"]["RR"].copy()
    for t in range(2, T - 1, 5):
        Qm, _ = np.linalg.qr(rng.normal(size=(2, 2)))
        Rneg[:, :, t] = Qm @ np.diag([-1.0, 0.5]) @ Qm.T
    cases["indef"] = dict(base="plain0", RR=Rneg)
    cases["indef_aug"] = dict(base="aug0", RR=Rneg)
    # R = [[a, b], [-b, a]] with |b| >> |B^T P B|: M has a complex pair, real part ~ a (+ / - by stage)
    Rc = np.zeros((2, 2, T))
    for t in range(T):
        a = 0.6 if t % 3 else -2.5
        Rc[:, :, t] = [[a, 3.0], [-3.0, a]]
    cases["complex"] = dict(base="plain1", RR=Rc)

    out = {}
    orig = np.linalg.eigvals
    for name, c in cases.items():
        full = dict(c)
        while "base" in full:
            b = cases[full.pop("base")]
            full = {**b, **full}
        TT = full.get("TT", full["AA"].shape[-1] if full["AA"].ndim == 3 else T)
        nreg = {"n": 0}
        cplx = {"pos": 0, "neg": 0}

        def tap(M):
            w = orig(M)
            if np.iscomplexobj(w):
                cplx["pos" if w.real[0] > 0 else "neg"] += 1
            if not np.all(w > 0):
                nreg["n"] += 1
            return w

        buf = io.StringIO()
        np.linalg.eigvals = tap
        try:
            with contextlib.redirect_stdout(buf):
                KK, PP, xx, uu = ref_opt.ltv_LQR(full["AA"], full["BB"], full["QQ"], full["RR"], full["SS"], full["QQf"],
                                                 TT, full["x0"], full.get("qq"), full.get("rr"), full.get("qqf"))
        finally:
            np.linalg.eigvals = orig
        aug = any(k in full for k in ("qq", "rr", "qqf"))
        assert buf.getvalue() == ("Augmented term!\n" if aug else "")
        assert np.isfinite(KK).all() and np.isfinite(PP).all() and np.isfinite(xx).all()
        for k, v in c.items():
            out["%s__%s" % (name, k)] = np.array(v) if k == "base" else v
        out["%s__TT" % name] = np.int64(TT)
        out.update({"%s__KK" % name: KK, "%s__PP" % name: PP, "%s__xx" % name: xx.copy(), "%s__uu" % name: uu.copy(),
                    "%s__n_regularised" % name: np.int64(nreg["n"])})
        print("  G12 %-10s T=%-3d aug=%d regularised stages %d, complex M (Re>0 / Re<0) %d / %d, max|KK| %.3g max|PP| %.3g"
              % (name, TT, aug, nreg["n"], cplx["pos"], cplx["neg"], np.abs(KK).max(), np.abs(PP).max()))
        if name.startswith("indef"):
            assert nreg["n"] > 0
        if name == "complex":
            assert cplx["pos"] > 0 and cplx["neg"] > 0 and nreg["n"] >= cplx["neg"]
    save("g12_ltv_general", cases=np.array(list(cases)), **out)


def step_wide_vectors():
    """G13: Dynamics.step (aircraft_simplified.py:263-393) with lmbd beyond G1's box: theta, gamma and theta-gamma over
    +-4 pi, at points within 1e-9 of every k pi/4 on both sides (where a quadrant of the argument reduction changes), a
    few angles in [2^20, 2^24] and their negatives, V from 0.05 to 300 (log-uniform); inputs and costates as G1."""
    rng = np.random.default_rng(20261017)
    dyn = ref_air.Dynamics()
    dyn.dt = 1e-3
    ks = np.arange(-16, 17) * (np.pi / 4)
    near = np.concatenate([ks - rng.uniform(1e-11, 1e-9, ks.size), ks + rng.uniform(1e-11, 1e-9, ks.size)])
    m = near.size
    wide = lambda n: rng.uniform(-4 * np.pi, 4 * np.pi, n)
    th = np.concatenate([near, wide(m), np.zeros(m)])
    ga = np.concatenate([wide(m), near, np.zeros(m)])
    th[2 * m:] = wide(m)
    ga[2 * m:] = th[2 * m:] - near                         # theta - gamma near k pi/4
    huge = rng.uniform(2.0 ** 20, 2.0 ** 24, 3)
    huge = np.concatenate([huge, -huge])
    th = np.concatenate([th, huge, rng.uniform(-3, 3, 6), huge[::-1]])
    ga = np.concatenate([ga, rng.uniform(-3, 3, 6), huge, huge])
    n = th.size
    X = np.stack([rng.uniform(-5, 20, n), rng.uniform(-3, 5, n), np.exp(rng.uniform(np.log(0.05), np.log(300), n)),
                  th, rng.uniform(-25, 25, n), ga], 1)
    X[:4, 2] = (0.05, 300.0, 0.05, 300.0)
    U = np.stack([rng.uniform(0, 900, n), rng.uniform(-100, 300, n)], 1)
    L = rng.normal(0, 50, (n, 6))
    xp = np.zeros((n, 6), np.float32); fx = np.zeros((n, 6, 6)); fu = np.zeros((n, 2, 6))
    fxx = np.zeros((n, 6, 6)); fuu = np.zeros((n, 2, 2)); fux = np.zeros((n, 2, 6))
    fxx3 = np.zeros((n, 6, 6, 6)); fux3 = np.zeros((n, 2, 6, 6)); fuu3 = np.zeros((n, 2, 2, 6))
    for i in range(n):
        xp[i], fx[i], fu[i], fxx[i], fuu[i], fux[i] = dyn.step(X[i], U[i], L[i])
        r = dyn.step(X[i], U[i])
        assert np.array_equal(r[0], xp[i])
        fxx3[i], fuu3[i], fux3[i] = r[3], r[4], r[5]
    assert np.isfinite(fx).all() and np.isfinite(fxx).all() and np.isfinite(xp).all()
    sel = np.r_[0:4, m - 2:m + 2, 3 * m:3 * m + 4]        # uncontracted tensors: extreme V, both sides of 0, huge angles
    save("g13_step_wide", x=X, u=U, lmbd=L, dt=np.float64(dyn.dt), xp=xp, fx=fx, fu=fu, fxx=fxx, fuu=fuu, fux=fux,
         sel3=sel, fxx3=fxx3[sel], fuu3=fuu3[sel], fux3=fux3[sel])


def sym_upper(M):
    """The symmetric matrix of M's upper triangle, exactly (not left to whether NumPy computes A @ A.T with syrk)."""
    return np.triu(M) + np.triu(M, 1).T


def dense_weights(p, seed=0):
    """The dense weights of tests/test_gpu_edges.py::_setup(dense=True): Q += A A^T (A ~ 1e-3 N(0, 1)), Q_T += A A^T
    (1e-2), R01 = R10 = 2e-7, each made exactly symmetric."""
    rng = np.random.default_rng(seed)
    Q, R, QT = p["QQt"].copy(), p["RRt"].copy(), p["QQT"].copy()
    for M, sc in ((Q, 1e-3), (QT, 1e-2)):
        A = rng.normal(size=(6, 6)) * sc
        M += A @ A.T
    R += np.array([[0.0, 2e-7], [2e-7, 0.0]])
    return sym_upper(Q), sym_upper(R), sym_upper(QT)


def dense_vectors():
    """G14: dense weights.  (a) dense symmetric Q, R, Q_T on the step problem at T = 500: NewtonMethod from the
    reference's own initial guess, 11 iterations (the Hessian switch at kk = 9 crossed), every iterate kept.  (b) the same
    with Q made non-symmetric by upper-triangle noise of 1e-3 of the diagonal scale (Q_T symmetric): the
    reference uses the full matrix (aircraft_simplified.py:61-68).  (c) the generic ltv_LQR (optcon.py:533-771) on one
    seeded problem whose per-stage Q and whose Qf are not symmetric, with affine terms."""
    p5 = step_problem(tf=1.0, dt=2e-3)
    xi, ui = p5["dyn"].get_initial_trajectory(p5["xx_ref"], p5["tt"])
    Q, R, QT = dense_weights(p5)
    # the scale of the noise: the mean diagonal entry of the dense part added to the driver's Q (~6e-6).  Scaled by
    # sqrt(Q_ii Q_jj) instead, the reference itself meets a NaN in eigvals within 11 iterations: the antisymmetric part
    # of P grows without bound through the Riccati recursion (|P| ~ 7e11 at kk = 0).  Even this noise moves the step by
    # O(1) of the input channels if Q is mirrored from its upper triangle.
    rng = np.random.default_rng(20261018)
    Qn = Q + np.triu(rng.normal(size=(6, 6)), 1) * 1e-3 * (Q - p5["QQt"]).diagonal().mean()
    assert not np.array_equal(Qn, Qn.T) and np.array_equal(Q, Q.T) and np.array_equal(QT, QT.T)
    n_it = 11
    for name, Qc in (("g14_dense_step_T500", Q), ("g14_dense_nonsym_q_step_T500", Qn)):
        p = dict(p5, QQt=Qc, RRt=R, QQT=QT)
        r, _ = run_newton(p, xi, ui, n_it, range(1, n_it + 1))
        assert int(r["n_done"]) == n_it, int(r["n_done"])
        save(name, QQt=Qc, RRt=R, QQT=QT, **r)
        print("  G14 %s: steps %s, trials %s, cost %r -> %r" % (name, r["stepsize"].tolist(), r["ntrials"].tolist(),
                                                               float(r["cost"][0]), float(r["cost"][-1])))
    # (c) generic ltv_LQR, T = 40: SPD-plus-noise Q_t (non-symmetric at every stage), non-symmetric Qf
    rng = np.random.default_rng(20261019)
    T = 40

    def spd(n, lo, hi):
        Qm, _ = np.linalg.qr(rng.normal(size=(n, n)))
        return Qm @ np.diag(rng.uniform(lo, hi, n)) @ Qm.T

    AA = np.stack([0.9 * np.linalg.qr(rng.normal(size=(6, 6)))[0] + 0.08 * rng.normal(size=(6, 6)) for _ in range(T)], -1)
    BB = 0.3 * rng.normal(size=(6, 2, T))
    QQ = np.stack([spd(6, 0.1, 2.0) + np.triu(0.3 * rng.normal(size=(6, 6)), 1) for _ in range(T)], -1)
    RR = np.stack([spd(2, 0.05, 1.0) for _ in range(T)], -1)
    SS = 0.05 * rng.normal(size=(2, 6, T))
    QQf = spd(6, 0.5, 5.0) + np.triu(0.5 * rng.normal(size=(6, 6)), 1)
    x0 = rng.normal(0, 1, 6)
    qq, rr, qqf = rng.normal(0, 1, (6, T)), rng.normal(0, 1, (2, T)), rng.normal(0, 1, 6)
    assert not any(np.array_equal(QQ[:, :, t], QQ[:, :, t].T) for t in range(T)) and not np.array_equal(QQf, QQf.T)
    nreg = {"n": 0}
    orig = np.linalg.eigvals

    def tap(M):
        w = orig(M)
        if not np.all(w > 0):
            nreg["n"] += 1
        return w

    buf = io.StringIO()
    np.linalg.eigvals = tap
    try:
        with contextlib.redirect_stdout(buf):
            KK, PP, xx, uu = ref_opt.ltv_LQR(AA, BB, QQ, RR, SS, QQf, T, x0, qq, rr, qqf)
    finally:
        np.linalg.eigvals = orig
    assert buf.getvalue() == "Augmented term!\n"
    assert np.isfinite(KK).all() and np.isfinite(PP).all() and np.isfinite(xx).all()
    print("  G14 ltv_nonsym T=%d regularised stages %d, max|KK| %.3g max|PP| %.3g, max|PP - PP^T| %.3g"
          % (T, nreg["n"], np.abs(KK).max(), np.abs(PP).max(), np.abs(PP - PP.transpose(1, 0, 2)).max()))
    save("g14_ltv_nonsym", AA=AA, BB=BB, QQ=QQ, RR=RR, SS=SS, QQf=QQf, x0=x0, qq=qq, rr=rr, qqf=qqf, TT=np.int64(T),
         KK=KK, PP=PP, xx=xx.copy(), uu=uu.copy(), n_regularised=np.int64(nreg["n"]))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "dense":
        return dense_vectors()
    if len(sys.argv) > 1 and sys.argv[1] == "gradient":
        return gradient_vectors()
    if len(sys.argv) > 1 and sys.argv[1] == "ltv_general":
        return ltv_general_vectors()
    if len(sys.argv) > 1 and sys.argv[1] == "step_wide":
        return step_wide_vectors()
    if len(sys.argv) > 1 and sys.argv[1] == "airfoil":     # only the fixture added in round 5
        return airfoil_vectors()
    if len(sys.argv) > 1 and sys.argv[1] == "config1":   # only the fixtures added in round 2
        return config1_full_solves()
    rng = np.random.default_rng(20260331)

    # ---------------- G1: Dynamics.step unit vectors ----------------
    dyn = ref_air.Dynamics()
    n = 64
    X = np.stack([rng.uniform(-5, 20, n), rng.uniform(-3, 5, n), rng.uniform(9, 23, n),
                  rng.uniform(-1.5, 1.5, n), rng.uniform(-25, 25, n), rng.uniform(-1.5, 1.5, n)], 1)
    U = np.stack([rng.uniform(0, 900, n), rng.uniform(-100, 300, n)], 1)
    L = rng.normal(0, 50, (n, 6))
    for dt in (1e-3, 2e-3):
        dyn.dt = dt
        xp = np.zeros((n, 6), np.float32); fx = np.zeros((n, 6, 6)); fu = np.zeros((n, 2, 6))
        fxx = np.zeros((n, 6, 6)); fuu = np.zeros((n, 2, 2)); fux = np.zeros((n, 2, 6))
        fxx3 = np.zeros((n, 6, 6, 6)); fux3 = np.zeros((n, 2, 6, 6)); fuu3 = np.zeros((n, 2, 2, 6))
        for i in range(n):
            xp[i], fx[i], fu[i], fxx[i], fuu[i], fux[i] = dyn.step(X[i], U[i], L[i])
            r = dyn.step(X[i], U[i])
            assert np.array_equal(r[0], xp[i])
            fxx3[i], fuu3[i], fux3[i] = r[3], r[4], r[5]
        save("g1_step_dt%g" % dt, x=X, u=U, lmbd=L, dt=np.float64(dt), xp=xp, fx=fx, fu=fu,
             fxx=fxx, fuu=fuu, fux=fux, fxx3=fxx3[:8], fuu3=fuu3[:8], fux3=fux3[:8])

    # ---------------- G2: Cost unit vectors ----------------
    ps = step_problem()
    pa = acro_problem()
    for tag, p in (("step", ps), ("acro", pa)):
        cst = ref_air.Cost(p["QQt"], p["RRt"], p["QQT"])
        XR = X + rng.normal(0, 1, X.shape)
        UR = U + rng.normal(0, 10, U.shape)
        ll = np.zeros(n); lx = np.zeros((n, 6)); lu = np.zeros((n, 2)); lT = np.zeros(n); lTx = np.zeros((n, 6))
        for i in range(n):
            r = cst.stagecost(X[i], U[i], XR[i], UR[i])
            ll[i], lx[i], lu[i] = r[0].item(), r[1].squeeze(), r[2].squeeze()
            assert np.array_equal(r[3], p["QQt"]) and np.array_equal(r[6], p["RRt"])
            assert not r[4].any() and not r[5].any()
            rT = cst.termcost(X[i], XR[i])
            lT[i], lTx[i] = rT[0].item(), rT[1].squeeze()
        save("g2_cost_" + tag, x=X, u=U, xr=XR, ur=UR, QQt=p["QQt"], RRt=p["RRt"], QQT=p["QQT"],
             ll=ll, lx=lx, lu=lu, llT=lT, lTx=lTx)

    # ---------------- problems + reference initial guesses ----------------
    save("problem_step_T1000", xxe=ps["xxe"], uue=ps["uue"].astype(np.float64), **problem_arrays(ps))
    save("problem_acro_T1000", xxe=pa["xxe"], uue=pa["uue"].astype(np.float64), **problem_arrays(pa))
    p5 = step_problem(tf=1.0, dt=2e-3)
    save("problem_step_T500", xxe=p5["xxe"], uue=p5["uue"].astype(np.float64), **problem_arrays(p5))

    xi_s, ui_s = ps["dyn"].get_initial_trajectory(ps["xx_ref"], ps["tt"])
    xi_a, ui_a = pa["dyn"].get_initial_trajectory(pa["xx_ref"], pa["tt"])
    xi_5, ui_5 = p5["dyn"].get_initial_trajectory(p5["xx_ref"], p5["tt"])

    # ---------------- G6/G5: Newton chains with per-iteration taps ----------------
    keep = (1, 2, 3, 6, 9, 10, 11, 12, 16, 20)
    c5, its5 = run_newton(p5, xi_5, ui_5, 20, keep)
    save("g6_chain_step_T500", **c5)
    cs, itss = run_newton(ps, xi_s, ui_s, 12, (1, 3, 10, 12))
    save("g6_chain_step_T1000", **cs)
    ca, itsa = run_newton(pa, xi_a, ui_a, 10, (1, 10))
    save("g6_chain_acro_T1000", **ca)

    # ---------------- G8: full solves (termination + returned index quirk) ----------------
    full5, itf5 = run_newton(p5, xi_5, ui_5, 199, ())
    nd = int(full5["n_done"])
    # the reference returns iterate n_done-2 (Q7); keep neighbours so the test can tell them apart
    for k in (nd - 2, nd - 1, nd):
        if 1 <= k <= len(itf5):
            full5["xx_it%d" % k], full5["uu_it%d" % k] = itf5[k - 1]
    save("g8_full_step_T500", **full5)
    print("full T500 solve: iterations printed =", nd, "ntrials", full5["ntrials"].tolist())

    # ---------------- G3: ltv_LQR cases (a) GN on initial guess (b) full Hessian on initial guess
    #                  (regularisation fires) (c) full Hessian near the optimum ----------------
    for tag, p, xx, uu, fh in (("a_gn_init_T1000", ps, xi_s, ui_s, 0),
                               ("b_full_init_T1000", ps, xi_s, ui_s, 1),
                               ("c_full_near_T500", p5, its5[15][0], its5[15][1], 1),
                               ("d_gn_init_T500", p5, xi_5, ui_5, 0)):
        r = lqr_case(p, xx, uu, fh)
        print("  G3", tag, "regularised stages:", int(r["n_regularised"]), "descent", float(r["descent"]))
        save("g3_lqr_" + tag, **r)

    # ---------------- G4: lqr_tracking on the reference's saved optimum ----------------
    xx_opt = np.load(os.path.join(REF, "Data", "xx_star.npy"))
    uu_opt = np.load(os.path.join(REF, "Data", "uu_star.npy"))
    dynl = ref_air.Dynamics()
    QQl = np.eye(6) * 0.01; QQl[1, 1] = 10; QQl[0, 0] = 10
    RRl = np.eye(2) * 1e-5
    for k, v in dict(dyn=dynl, ns=6, ni=2, QQt=QQl, RRt=RRl, QQT=QQl.copy()).items():
        setattr(ref_lqr, k, v)
    ttl = np.linspace(0, 1, xx_opt.shape[1])
    xx_reg, uu_reg = ref_lqr.lqr_tracking(xx_opt, uu_opt, ttl)
    TT = xx_opt.shape[1]
    AA = np.zeros((6, 6, TT)); BB = np.zeros((6, 2, TT))
    for t in range(TT):
        _, fx, fu = dynl.step(xx_opt[:, t], uu_opt[:, t])[0:3]
        AA[:, :, t] = fx.T; BB[:, :, t] = fu.T
    KK, PP, lx, lu = ref_lqr.ltv_LQR(AA, BB, QQl, RRl, np.zeros((2, 6, TT)), QQl.copy(), TT,
                                     np.ones(6) * 0.1, None, None, None)
    KK2 = ref_opt.ltv_LQR(AA, BB, QQl, RRl, np.zeros((2, 6, TT)), QQl.copy(), TT,
                          np.ones(6) * 0.1, None, None, None)[0]
    assert np.array_equal(KK, KK2)
    save("g4_lqr_tracking", xx_opt=xx_opt, uu_opt=uu_opt, QQt=QQl, RRt=RRl, QQT=QQl, dt=np.float64(dynl.dt),
         xx_reg=xx_reg, uu_reg=uu_reg, KK=KK, PP_s=PP[:, :, ::50].copy(), lin_xx=lx, lin_uu=lu)
    # acrobatic optimum too (input fixture for config 3/5)
    save("data_acrobatic_star", xx_star=np.load(os.path.join(REF, "Data", "xx_star_acrobatic.npy")),
         uu_star=np.load(os.path.join(REF, "Data", "uu_star_acrobatic.npy")))

    # ---------------- G9: perturbed-x0 mini-batch, config-2 generation rule ----------------
    Bm = 8
    rng2 = np.random.default_rng(20260401)
    sig = np.array([0.5, 0.5, 0.5, 0.05, 0.1, 0.05])
    nit = 4
    x0s = p5["xx_ref"][:, 0][None, :] + rng2.normal(0, 1, (Bm, 6)) * sig
    XI = np.zeros((Bm, 6, p5["TT"])); UI = np.zeros((Bm, 2, p5["TT"]))
    XO = np.zeros((Bm, 6, p5["TT"])); UO = np.zeros((Bm, 2, p5["TT"]))
    CO = np.zeros((Bm, nit)); DE = np.zeros((Bm, nit)); ST = np.zeros((Bm, nit))
    for b in range(Bm):
        xr = p5["xx_ref"].copy(); xr[:, 0] = x0s[b]
        XI[b], UI[b] = p5["dyn"].get_initial_trajectory(xr, p5["tt"])
        r, its = run_newton(p5, XI[b], UI[b], nit, ())
        XO[b], UO[b] = its[nit - 1]
        CO[b], DE[b], ST[b] = r["cost"], r["descent"], r["stepsize"]
    config1_full_solves()
    airfoil_vectors()
    save("g9_minibatch_step_T500", x0=x0s, xx_init=XI, uu_init=UI, xx_out=XO.astype(np.float32),
         x0_out=XO[:, :, 0].copy(), uu_out=UO, cost=CO, descent=DE, stepsize=ST, n_iters=np.int64(nit))


if __name__ == "__main__":
    main()
