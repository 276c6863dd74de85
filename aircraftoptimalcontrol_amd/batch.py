"""Batched host API over the C-ABI (include/aoc.h).

torch-ROCm is used for device memory, streams and (in bench.py) torch.distributed only; every
numerical operation of the hot path is a HIP kernel of libaoc_hip.so.  Arrays at this level use the
reference's per-trajectory conventions stacked over the batch: xx (B,6,T), uu (B,2,T), float64.
"""
import ctypes as C
import os
import time

import numpy as np

from . import _lib
from ._lib import AocError, Model, Params, Problem, check, lib

TILE = _lib.AOC_TILE


def default_model(dt=1e-3):
    """Dynamics.__init__ constants (reference aircraft_simplified.py:108-118)."""
    return Model(0.1716, 2.395, 3.256, 12.0, 9.81, 0.61, 1.2, 0.24, dt)


def make_params(max_iters=200, stepsize_0=1e-2, cc=0.5, beta=0.7, armijo_maxiters=20, term_cond=-1e-6,
                hessian_switch=8):
    """NewtonMethod constructor defaults (reference optcon.py:335-339); term_cond is the value the
    reference hard-codes (-1e-6, optcon.py:368), not the ignored constructor argument."""
    return Params(int(max_iters), int(armijo_maxiters), float(stepsize_0), float(cc), float(beta),
                  float(term_cond), int(hessian_switch), 0)


def _torch():
    return _lib.require_gpu()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_f64(a, device):
    torch = _torch()
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


class BatchProblem:
    """Dynamics constants + Cost weights + reference curves on one GPU.

    Mirrors what NewtonMethod.__init__ captures (reference optcon.py:335-339).  xx_ref (6,T) / uu_ref (2,T): one
    curve shared by every trajectory of the batch (B instances of the same NewtonMethod).  xx_ref (B,6,T) / uu_ref
    (B,2,T): one curve per trajectory (B NewtonMethod instances with their own references: different manoeuvres in
    one batch, MPC instances tracking different targets); the batch size is then fixed to B."""

    def __init__(self, QQt, RRt, QQT, xx_ref, uu_ref, dt, model=None, device="cuda:0"):
        torch = _torch()
        self.device = torch.device(device)
        xx_ref = np.ascontiguousarray(xx_ref, dtype=np.float64)
        uu_ref = np.ascontiguousarray(uu_ref, dtype=np.float64)
        self.per_traj = xx_ref.ndim == 3
        if self.per_traj:
            if xx_ref.shape[1] != 6 or uu_ref.shape != (xx_ref.shape[0], 2, xx_ref.shape[2]):
                raise ValueError("per-trajectory references: xx_ref must be (B,6,T) and uu_ref (B,2,T)")
        elif xx_ref.ndim != 2 or xx_ref.shape[0] != 6 or uu_ref.shape != (2, xx_ref.shape[1]):
            raise ValueError("xx_ref must be (6,T) and uu_ref (2,T)")
        self.T = int(xx_ref.shape[-1])
        self.QQt = np.ascontiguousarray(QQt, dtype=np.float64).reshape(6, 6)
        self.RRt = np.ascontiguousarray(RRt, dtype=np.float64).reshape(2, 2)
        self.QQT = np.ascontiguousarray(QQT, dtype=np.float64).reshape(6, 6)
        self.model = model if model is not None else default_model(dt)
        self.model.dt = float(dt)
        self.xx_ref, self.uu_ref = xx_ref, uu_ref
        self.ref_T = 0          # samples per trajectory of a per-trajectory `ref` array (0 = T) and element offset of
        self.ref_offset = 0     #  the window in use: a long curve on the device, a window of it per call (mpc.py)
        if self.per_traj:
            self.B_ref = int(xx_ref.shape[0])
            self.ref = pack(np.concatenate([xx_ref, uu_ref], axis=1), self.device)    # tiled, C = 8
        else:
            self.B_ref = None
            ref = np.concatenate([xx_ref, uu_ref], axis=0).T.copy()  # [T][8]
            self.ref = torch.from_numpy(ref).to(self.device)

    def c_problem(self, B, stream=None, x_in_f32=0, x_out_f32=0, x_is_rollout=0):
        torch = _torch()
        if self.per_traj and int(B) != self.B_ref:
            raise ValueError("this problem carries %d per-trajectory reference curves; batch of %d asked" % (self.B_ref, B))
        p = Problem()
        p.x_in_f32, p.x_out_f32 = int(x_in_f32), int(x_out_f32)
        p.ref_per_traj, p.ref_T = int(self.per_traj), int(self.ref_T)
        p.x_is_rollout = int(x_is_rollout)
        p.model = self.model
        p.QQt[:] = self.QQt.ravel().tolist()
        p.RRt[:] = self.RRt.ravel().tolist()
        p.QQT[:] = self.QQT.ravel().tolist()
        p.B, p.T = int(B), self.T
        p.ref = self.ref.data_ptr() + int(self.ref_offset) * self.ref.element_size()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        p.stream = s.cuda_stream
        return p


def ntiles(B):
    return (B + TILE - 1) // TILE


def alloc_tiled(B, T, Cc, device, zero=False, f32=False):
    torch = _torch()
    shape = (ntiles(B), T, Cc, TILE)
    return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32 if f32 else torch.float64, device=device)


def pack(a_bct, device=None, f32=False):
    """(B,C,T) fp64 -> tiled [ntiles][T][C][64] on the device (aoc_pack / aoc_pack_f32)."""
    torch = _torch()
    if device is None:
        device = a_bct.device if isinstance(a_bct, torch.Tensor) and a_bct.is_cuda else "cuda:0"
    src = _dev_f64(a_bct, device)
    B, Cc, T = src.shape
    dst = alloc_tiled(B, T, Cc, src.device, f32=f32)
    fn = lib().aoc_pack_f32 if f32 else lib().aoc_pack
    check(fn(B, T, Cc, _ptr(src), _ptr(dst), C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)), "aoc_pack")
    return dst


def unpack(tiled, B):
    """tiled (fp64 or float32) -> (B,C,T) fp64 torch tensor on the device (aoc_unpack / aoc_unpack_f32)."""
    torch = _torch()
    nt, T, Cc, _ = tiled.shape
    dst = torch.empty((B, Cc, T), dtype=torch.float64, device=tiled.device)
    fn = lib().aoc_unpack_f32 if tiled.dtype == torch.float32 else lib().aoc_unpack
    check(fn(B, T, Cc, _ptr(tiled), _ptr(dst), C.c_void_p(torch.cuda.current_stream(tiled.device).cuda_stream)),
          "aoc_unpack")
    return dst


def unpack_gains(Kt, B):
    """K~ as aoc_backward writes it — per tile and sample seven columns, the two rows of a column side by side:
    [ntiles][T][7][64][2] — -> (B,2,7,T) fp64 torch tensor on the device (the reference's KK[:, :, t], optcon.py:751)."""
    nt, T = Kt.shape[0], Kt.shape[1]
    v = Kt.reshape(nt, T, 7, TILE, 2)
    return v.permute(0, 3, 4, 2, 1).reshape(nt * TILE, 2, 7, T)[:B]


def unpack_vec(v, B):
    """[ntiles][C][64] -> (B,C)"""
    return v.permute(0, 2, 1).reshape(-1, v.shape[1])[:B]


def pack_vec(a_bc, device):
    """(B,C) per-trajectory vectors -> [ntiles][C][64]."""
    torch = _torch()
    a = _dev_f64(a_bc, device)
    B, Cc = a.shape
    nt = ntiles(B)
    if nt * TILE != B:
        a = torch.cat([a, a[-1:].expand(nt * TILE - B, Cc)], 0)
    return a.reshape(nt, TILE, Cc).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------
# unit level
# ------------------------------------------------------------------------------------------------
def step_batch(model, x, u, lmbd=None, device="cuda:0"):
    """Dynamics.step for n points (reference aircraft_simplified.py:263-393).
    Returns numpy (xp, fx, fu, fxx, fuu, fux); the last three are None without lmbd."""
    torch = _torch()
    two_d = lambda a: a if isinstance(a, torch.Tensor) else np.atleast_2d(a)
    xd, ud = _dev_f64(two_d(x), device), _dev_f64(two_d(u), device)
    n = xd.shape[0]
    ld = None if lmbd is None else _dev_f64(two_d(lmbd), device)
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device=xd.device)
    xp, fx, fu = mk(n, 6), mk(n, 6, 6), mk(n, 2, 6)
    fxx, fuu, fux = (mk(n, 6, 6), mk(n, 2, 2), mk(n, 2, 6)) if ld is not None else (None, None, None)
    st = C.c_void_p(torch.cuda.current_stream(xd.device).cuda_stream)
    check(lib().aoc_step_batch(C.byref(model), n, _ptr(xd), _ptr(ud), _ptr(ld), _ptr(xp), _ptr(fx), _ptr(fu),
                               _ptr(fxx), _ptr(fuu), _ptr(fux), st), "aoc_step_batch")
    torch.cuda.synchronize(xd.device)
    out = [xp, fx, fu, fxx, fuu, fux]
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def cost_batch(problem, x, u, xr, ur):
    """Cost.stagecost/termcost for n points (reference aircraft_simplified.py:25-97).
    Returns numpy (ll, lx, lu, llT, lTx)."""
    torch = _torch()
    dev = problem.device
    xd, ud, xrd, urd = (_dev_f64(np.atleast_2d(a), dev) for a in (x, u, xr, ur))
    n = xd.shape[0]
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    ll, lx, lu, llT, lTx = mk(n), mk(n, 6), mk(n, 2), mk(n), mk(n, 6)
    p = problem.c_problem(n)
    check(lib().aoc_cost_batch(C.byref(p), n, _ptr(xd), _ptr(ud), _ptr(xrd), _ptr(urd), _ptr(ll), _ptr(lx), _ptr(lu),
                               _ptr(llT), _ptr(lTx), C.c_void_p(p.stream)), "aoc_cost_batch")
    torch.cuda.synchronize(dev)
    return tuple(o.cpu().numpy() for o in (ll, lx, lu, llT, lTx))


# ------------------------------------------------------------------------------------------------
# iteration level
# ------------------------------------------------------------------------------------------------
class NewtonBatchSolver:
    """B independent NewtonMethod.optimize instances (reference optcon.py:341-529) on one GPU.

    Device state (tiled): three (x,u) iterate buffers in rotation — states as float32 (lossless: every
    propagated state of the reference is a float32 value, aircraft_simplified.py:300; sample 0 lives in
    the fp64 x0 array), inputs as fp64 — the K~/du workspace and per-trajectory scalars.  A
    caller-supplied initial iterate whose samples are not float32 values is kept in an extra fp64
    buffer and read from there by the first iteration.  `iterate(kk)` = one outer iteration for every
    trajectory; `solve()` adds the reference's termination and return-index behaviour per trajectory."""

    def __init__(self, problem, B, params=None, arena=None):
        """arena (vmm.Arena, optional): where the big streams of the solver live — the three iterate buffers and the
        K~/du workspace — instead of torch's allocator; `arena_layout` records what was taken.  The write-heavy streams
        (workspace first, then the iterate buffers) each start on a physical handle of their own (new_handle)."""
        torch = _torch()
        self.problem, self.B, self.T = problem, int(B), problem.T
        self.params = params if params is not None else make_params()
        dev = problem.device
        self.nt = ntiles(self.B)
        self.Bp = self.nt * TILE
        self.arena = arena
        ws_elems = (lib().aoc_workspace_bytes(self.B, self.T) + 7) // 8
        if arena is not None:
            self.ws = arena.take((ws_elems,), "float64", new_handle=True)
            self.xb = [arena.take((self.nt, self.T, 6, TILE), "float32", zero=True, new_handle=True) for _ in range(3)]
            self.ub = [arena.take((self.nt, self.T, 2, TILE), "float64", zero=True, new_handle=True) for _ in range(3)]
        else:
            self.xb = [alloc_tiled(B, self.T, 6, dev, zero=True, f32=True) for _ in range(3)]
            self.ub = [alloc_tiled(B, self.T, 2, dev, zero=True) for _ in range(3)]
            self.ws = torch.empty(ws_elems, dtype=torch.float64, device=dev)
        self.x64 = None            # fp64 copy of a caller-supplied initial iterate (only if needed)
        self.cur_is64 = False      # the current iterate is the one in self.x64
        self.cur_rollout = False   # the current iterate's states are the rollout of its inputs (written by the library)
        self.x_init = None         # (B,6,T) fp64: what set_initial() was given (returned verbatim if a
        self.u_init = None         #  trajectory stops at kk = 1, optcon.py:500-504)
        f = lambda: torch.zeros(self.Bp, dtype=torch.float64, device=dev)
        self.J = [f(), f()]
        self.descent, self.stepsize = f(), f()
        self.ntrials = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        self.x0 = torch.zeros((self.nt, 6, TILE), dtype=torch.float64, device=dev)
        self.spec_max = int(lib().aoc_spec_max())
        self.cur = 0      # index of the buffer holding the current iterate
        self.kk = 0       # outer-iteration index of the current iterate
        self.jcur = 0

    @property
    def n_spec(self):
        """Armijo trials riding along in the forward pass: what aoc_newton_iterate uses for this batch size under the
        aoc_tuning of the moment."""
        return int(lib().aoc_default_nspec(self.B, int(self.params.armijo_maxiters)))

    # -- problem struct with the current stream and the element types of this call's state arrays
    def _p(self, x_in_f32=1, x_out_f32=1):
        return self.problem.c_problem(self.B, x_in_f32=x_in_f32, x_out_f32=x_out_f32, x_is_rollout=self.cur_rollout)

    def _xin(self):
        """(pointer, is_f32) of the current iterate's state array"""
        return (self.x64, 0) if self.cur_is64 else (self.xb[self.cur], 1)

    def set_initial(self, xx_init, uu_init):
        """xx[:,:,0], uu[:,:,0] = xx_init, uu_init; x0 = xx_init[:,0] (reference optcon.py:395-398)."""
        torch = _torch()
        dev = self.problem.device
        xi, ui = _dev_f64(xx_init, dev), _dev_f64(uu_init, dev)
        if tuple(xi.shape) != (self.B, 6, self.T) or tuple(ui.shape) != (self.B, 2, self.T):
            raise ValueError("xx_init must be (B,6,T)=(%d,6,%d) and uu_init (B,2,T)" % (self.B, self.T))
        self.x_init, self.u_init = xi, ui
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.x0.copy_(pack_vec(xi[:, :, 0], dev))
        tail = xi[:, :, 1:]
        self.cur_is64 = not bool(torch.equal(tail.to(torch.float32).to(torch.float64), tail))
        if self.cur_is64:
            if self.x64 is None:
                self.x64 = alloc_tiled(self.B, self.T, 6, dev)
            check(lib().aoc_pack(self.B, self.T, 6, _ptr(xi), _ptr(self.x64), st), "aoc_pack")
        check(lib().aoc_pack_f32(self.B, self.T, 6, _ptr(xi), _ptr(self.xb[0]), st), "aoc_pack_f32")
        check(lib().aoc_pack(self.B, self.T, 2, _ptr(ui), _ptr(self.ub[0]), st), "aoc_pack")
        self.cur, self.kk, self.jcur, self.cur_rollout = 0, 0, 0, False
        self.status.zero_()
        x, f32 = self._xin()
        p = self._p(f32)
        check(lib().aoc_traj_cost(C.byref(p), _ptr(x), _ptr(self.ub[0]), _ptr(self.x0), _ptr(self.J[0])), "aoc_traj_cost")

    def set_initial_from_x0(self, x0, kp=5.0, kt=2.5):
        """Initial guess by the reference's P-controller law (aircraft_simplified.py:134-147) rolled out
        on the device from x0 (B,6), straight into the iterate buffers."""
        dev = self.problem.device
        self.x0.copy_(pack_vec(x0, dev))
        self.x_init = self.u_init = None
        self.cur_is64 = False
        p = self._p()
        check(lib().aoc_initial_trajectory(C.byref(p), float(kp), float(kt), _ptr(self.x0), _ptr(self.xb[0]),
                                           _ptr(self.ub[0])), "aoc_initial_trajectory")
        self.cur, self.kk, self.jcur, self.cur_rollout = 0, 0, 0, True
        self.status.zero_()
        check(lib().aoc_traj_cost(C.byref(p), _ptr(self.xb[0]), _ptr(self.ub[0]), _ptr(self.x0), _ptr(self.J[0])),
              "aoc_traj_cost")

    def set_initial_from_rollout(self, x0, uu):
        """Initial iterate = the open-loop rollout of uu (B,2,T) from x0 (B,6) (get_update with no direction,
        optcon.py:176-200): the warm start of BASELINE configs[2] from a saved optimum, rolled out on the device."""
        torch = _torch()
        dev = self.problem.device
        self.x0.copy_(pack_vec(x0, dev))
        ut = pack(uu, dev)
        self.x_init = self.u_init = None
        self.cur_is64 = False
        self.status.zero_()
        p = self._p()
        check(lib().aoc_rollout_cost(C.byref(p), _ptr(self.x0), _ptr(ut), None, None, _ptr(self.xb[0]), _ptr(self.ub[0]),
                                     _ptr(self.J[0]), _ptr(self.status)), "aoc_rollout_cost")
        self.cur, self.kk, self.jcur, self.cur_rollout = 0, 0, 0, True

    def iterate(self, kk=None):
        """One outer iteration (steps A-G of SURVEY 3.2) for every trajectory; asynchronous."""
        if kk is None:
            kk = self.kk
        x, f32 = self._xin()
        p = self._p(f32)
        c, n = self.cur, (self.cur + 1) % 3
        jc, jn = self.jcur, 1 - self.jcur
        check(lib().aoc_newton_iterate(C.byref(p), C.byref(self.params), int(kk), _ptr(x), _ptr(self.ub[c]),
                                       _ptr(self.x0), _ptr(self.J[jc]), _ptr(self.ws), self.ws.numel() * 8, _ptr(self.xb[n]),
                                       _ptr(self.ub[n]), _ptr(self.J[jn]), _ptr(self.descent), _ptr(self.stepsize),
                                       _ptr(self.ntrials), _ptr(self.status)), "aoc_newton_iterate")
        self.cur, self.jcur, self.kk, self.cur_is64, self.cur_rollout = n, jn, kk + 1, False, True

    PASSES = ("backward", "forward", "linesearch_search", "linesearch_update")

    def _carve(self):
        """The workspace as aoc_newton_iterate lays it out: K~ | du | trial costs | line-search scratch | candidate store
        -> (Kt, du, J_trial, scratch, scratch bytes, n_spec, cand or None, cand bytes).  n_spec and the number of stored
        candidates are asked from the library at call time (aoc_default_nspec / aoc_default_ncand follow aoc_tuning), and
        the candidate store is handed over only if the workspace has room for it — as aoc_newton_iterate decides."""
        l = lib()
        nel14 = l.aoc_tiled_elems(self.B, self.T, 14)
        nel2 = l.aoc_tiled_elems(self.B, self.T, 2)
        Kt, du = self.ws[:nel14], self.ws[nel14:nel14 + nel2]
        o = nel14 + nel2
        Jt = self.ws[o:o + self.spec_max * self.Bp]
        o += self.spec_max * self.Bp
        scratch = self.ws[o:]
        sbytes = int(l.aoc_linesearch_scratch_bytes(self.B, self.T))
        sb = (sbytes + 255) // 256 * 256
        nsp = int(l.aoc_default_nspec(self.B, int(self.params.armijo_maxiters)))
        ncand = int(l.aoc_default_ncand(self.B, nsp, int(self.params.armijo_maxiters)))
        cbytes = int(l.aoc_candidate_bytes(self.B, self.T, ncand)) if ncand else 0
        cand = None
        if ncand and sb + cbytes <= scratch.numel() * 8:
            cand = scratch[sb // 8:]
        else:
            cbytes = 0
        return Kt, du, Jt, scratch, sbytes, nsp, cand, cbytes

    def iterate_passes(self, kk=None, between=None):
        """The launches of iterate(), issued pass by pass through the four entry points aoc_newton_iterate is made of:
        backward | forward | line-search rounds (aoc_linesearch_search) | final rollout (aoc_linesearch_update).
        between(i), if given, is called on the host before pass i (i indexing PASSES) and once more, with i = 4, after
        the last one — where a caller records events on the launch stream or makes it wait for another stream."""
        torch = _torch()
        if kk is None:
            kk = self.kk
        x, f32 = self._xin()
        p = self._p(f32)
        prm = self.params
        c, n = self.cur, (self.cur + 1) % 3
        jc, jn = self.jcur, 1 - self.jcur
        Kt, du, Jt, scratch, sbytes, nsp, cand, cbytes = self._carve()
        between = between or (lambda i: None)
        between(0)
        # (what lies behind K~ in the workspace is free until the forward pass: scratch of the backward pass, as in aoc_newton_iterate)
        check(lib().aoc_backward(C.byref(p), int(kk > prm.hessian_switch), _ptr(x), _ptr(self.ub[c]), _ptr(self.x0),
                                 _ptr(Kt), None, _ptr(self.status), _ptr(du), (self.ws.numel() - Kt.numel()) * 8), "aoc_backward")
        between(1)
        check(lib().aoc_forward(C.byref(p), C.byref(prm), nsp, _ptr(x), _ptr(self.ub[c]), _ptr(self.x0),
                                _ptr(Kt), _ptr(du), _ptr(self.descent), _ptr(Jt), _ptr(self.status), _ptr(cand), cbytes,
                                _ptr(self.ntrials)), "aoc_forward")
        between(2)
        check(lib().aoc_linesearch_search(C.byref(p), C.byref(prm), nsp, _ptr(self.ub[c]), _ptr(self.x0), _ptr(du),
                                          _ptr(self.J[jc]), _ptr(self.descent), _ptr(Jt), _ptr(self.stepsize),
                                          _ptr(self.ntrials), _ptr(scratch), sbytes), "aoc_linesearch_search")
        between(3)
        check(lib().aoc_linesearch_update(C.byref(p), C.byref(prm), _ptr(self.ub[c]), _ptr(self.x0), _ptr(du),
                                          _ptr(self.xb[n]), _ptr(self.ub[n]), _ptr(self.J[jn]), _ptr(self.stepsize),
                                          _ptr(self.ntrials), _ptr(self.status), _ptr(scratch), sbytes, nsp, _ptr(Jt),
                                          _ptr(cand), cbytes), "aoc_linesearch_update")
        between(4)
        self.cur, self.jcur, self.kk, self.cur_is64, self.cur_rollout = n, jn, kk + 1, False, True

    def iterate_timed(self, kk=None):
        """iterate_passes() with HIP events recorded on the launch stream between the passes.  Returns the five events;
        read them after a synchronize with ev[i].elapsed_time(ev[i+1]) [ms], i indexing PASSES."""
        torch = _torch()
        st = torch.cuda.current_stream(self.problem.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        self.iterate_passes(kk, lambda i: ev[i].record(st))
        return ev

    # -- results ---------------------------------------------------------------------------------
    def direction(self):
        """du (B,2,T) of the last iteration (it stays in the workspace until the next one)."""
        nel14 = lib().aoc_tiled_elems(self.B, self.T, 14)
        nel2 = lib().aoc_tiled_elems(self.B, self.T, 2)
        return unpack(self.ws[nel14:nel14 + nel2].view(self.nt, self.T, 2, TILE), self.B).cpu().numpy()

    def previous_inputs(self):
        """uu (B,2,T) of the iterate the last iteration started from (the buffers rotate over three slots)."""
        return unpack(self.ub[(self.cur - 1) % 3], self.B).cpu().numpy()

    def _unpack_iterate(self, i):
        """(B,6,T), (B,2,T) fp64 device tensors of buffer i, sample 0 restored from the fp64 x0."""
        if self.cur_is64 and i == self.cur:
            xx = unpack(self.x64, self.B)
        else:
            xx = unpack(self.xb[i], self.B)
            xx[:, :, 0] = unpack_vec(self.x0, self.B)
        return xx, unpack(self.ub[i], self.B)

    def current(self):
        """Current iterate as numpy (B,6,T), (B,2,T)."""
        xx, uu = self._unpack_iterate(self.cur)
        return xx.cpu().numpy(), uu.cpu().numpy()

    def scalars(self):
        """Per-trajectory scalars of the LAST iteration: cost of the iterate it started from, descent,
        accepted step, number of Armijo trials, cost of the new iterate, status flags."""
        B = self.B
        return dict(cost=self.J[1 - self.jcur][:B].cpu().numpy(), descent=self.descent[:B].cpu().numpy(),
                    stepsize=self.stepsize[:B].cpu().numpy(), ntrials=self.ntrials[:B].cpu().numpy(),
                    cost_new=self.J[self.jcur][:B].cpu().numpy(), status=self.status[:B].cpu().numpy())

    def join(self):
        """(interface shared with TwoStreamNewtonSolver: one stream, nothing to wait for)"""

    def summary_tensors(self):
        """(cost of the newest iterate, descent, trial count) of every trajectory as device tensors."""
        B = self.B
        return self.J[self.jcur][:B], self.descent[:B], self.ntrials[:B]

    def summary(self, out=None, accumulate=False):
        """sharding.SUMMARY_FIELDS of this batch as five fp64 scalars on the device, by aoc_summary (one kernel, fixed
        reduction order); accumulate: added to what `out` holds.  What the path's one collective reduces."""
        torch = _torch()
        dev = self.problem.device
        if out is None:
            out = torch.zeros(5, dtype=torch.float64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib().aoc_summary(self.B, _ptr(self.J[self.jcur]), _ptr(self.descent), _ptr(self.ntrials), _ptr(out),
                                int(bool(accumulate)), st), "aoc_summary")
        return out

    def run_fixed(self, n_iters, kk0=None, record=True):
        """n_iters iterations for every trajectory, no early exit (the bench mode)."""
        hist = []
        if kk0 is not None:
            self.kk = kk0
        for _ in range(n_iters):
            self.iterate()
            if record:
                hist.append(self.scalars())
        return hist

    def _compacted(self, keep):
        """A new solver holding only the trajectories `keep` (device index tensor into this one): their
        current and previous iterate, x0, current cost and status."""
        torch = _torch()
        n, dev = self.B, self.problem.device
        m = int(keep.numel())
        nw = type(self)(self.problem, m, self.params)   # a GradientBatchSolver stays one (its iterate() differs)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for src, dst in (((self.cur - 1) % 3, 0), (self.cur, 1)):   # previous -> slot 0, current -> slot 1
            xs = unpack(self.xb[src], n)[keep].contiguous()
            us = unpack(self.ub[src], n)[keep].contiguous()
            check(lib().aoc_pack_f32(m, self.T, 6, _ptr(xs), _ptr(nw.xb[dst]), st), "aoc_pack_f32")
            check(lib().aoc_pack(m, self.T, 2, _ptr(us), _ptr(nw.ub[dst]), st), "aoc_pack")
        nw.x0.copy_(pack_vec(unpack_vec(self.x0, n)[keep], dev))
        nw.J[0][:m] = self.J[self.jcur][:n][keep]
        nw.status[:m] = self.status[:n][keep]
        if self.x_init is not None:
            nw.x_init, nw.u_init = self.x_init[keep], self.u_init[keep]
        nw.cur, nw.jcur, nw.kk, nw.cur_is64, nw.cur_rollout = 1, 0, self.kk, False, True
        return nw

    def solve(self, verbose=False, callback=None, compact=True, compact_below=0.5, compact_min=2048):
        """NewtonMethod.optimize semantics per trajectory (reference optcon.py:415-505):
        iterate kk = 0..max_iters-2; a trajectory stops at the first kk with descent >= term_cond and
        then returns iterate kk-1 (python index -1 = an all-zero history slot when kk == 0); without
        convergence it returns the last computed iterate; finally uu_star[:,-1] = uu_star[:,-2].
        compact: once fewer than `compact_below` of the trajectories in flight are still iterating (and
        more than `compact_min` are in flight) the active ones are re-packed into a smaller batch, so
        that converged trajectories stop costing passes; results do not depend on it.
        Returns dict(xx_star (B,6,T), uu_star (B,2,T), iters (B,), converged, status, history of per-iteration
        scalars (B,n_iter), NaN / -1 where a trajectory was no longer iterating)."""
        torch = _torch()
        B, prm, T = self.B, self.params, self.T
        dev = self.problem.device
        out_x = torch.zeros((B, 6, T), dtype=torch.float64, device=dev)
        out_u = torch.zeros((B, 2, T), dtype=torch.float64, device=dev)
        g_iters = torch.zeros(B, dtype=torch.int32, device=dev)
        g_conv = torch.zeros(B, dtype=torch.bool, device=dev)
        g_status = torch.zeros(B, dtype=torch.int32, device=dev)
        hist = dict(cost=[], descent=[], stepsize=[], ntrials=[])

        def fresh(sv):
            act = torch.zeros(sv.Bp, dtype=torch.bool, device=dev)
            act[:sv.B] = True
            return dict(active=act, ret=torch.full((sv.Bp,), -2, dtype=torch.int32, device=dev),
                        res_x=torch.zeros_like(sv.xb[0]), res_u=torch.zeros_like(sv.ub[0]))

        def flush(sv, gidx, L, final_kk=None):
            """write the results of this generation's finished trajectories into the global arrays"""
            n = sv.B
            if final_kk is not None:  # still iterating at the end: the last computed iterate (index max_iters-1)
                m = L["active"].reshape(sv.nt, 1, 1, TILE)
                L["res_x"] = torch.where(m, sv.xb[sv.cur], L["res_x"])
                L["res_u"] = torch.where(m, sv.ub[sv.cur], L["res_u"])
                L["ret"] = torch.where(L["active"], torch.full_like(L["ret"], final_kk + 1), L["ret"])
            ret = L["ret"][:n]
            done = ret != -2
            if bool(done.any()):
                xs, us = unpack(L["res_x"], n), unpack(L["res_u"], n)
                real = ret >= 0
                xs[:, :, 0] = torch.where(real[:, None], unpack_vec(sv.x0, n), xs[:, :, 0])  # sample 0 is the fp64 x0
                if sv.x_init is not None:  # index 0 is the caller's initial iterate, verbatim
                    is0 = ret == 0
                    xs = torch.where(is0[:, None, None], sv.x_init, xs)
                    us = torch.where(is0[:, None, None], sv.u_init, us)
                us[:, :, -1] = us[:, :, -2]  # optcon.py:505
                tgt = gidx[done]
                out_x[tgt], out_u[tgt] = xs[done], us[done]
            if final_kk is not None:  # status of the trajectories that never stopped
                live = L["active"][:n]
                g_status[gidx[live]] = sv.status[:n][live]

        sv, gidx = self, torch.arange(B, device=dev)
        L = fresh(sv)
        last = -1
        for kk in range(prm.max_iters - 1):
            sv.iterate(kk)
            last = kk
            n = sv.B
            sc = sv.scalars()
            act = L["active"]
            was = act[:n].cpu().numpy()                 # iterating at the start of this iteration
            gnp = gidx.cpu().numpy()[was]
            for k_ in hist:
                full = np.full(B, -1, dtype=np.int64) if k_ == "ntrials" else np.full(B, np.nan)
                full[gnp] = sc[k_][was]
                hist[k_].append(full)
            conv = act & (sv.descent >= prm.term_cond)
            g_iters[gidx[act[:n]]] = kk + 1
            if bool(conv.any()):
                m = conv.reshape(sv.nt, 1, 1, TILE)
                if kk >= 1:  # iterate kk-1 lives two buffers behind the newest
                    L["res_x"] = torch.where(m, sv.xb[(sv.cur + 1) % 3], L["res_x"])
                    L["res_u"] = torch.where(m, sv.ub[(sv.cur + 1) % 3], L["res_u"])
                # kk == 0: xx[:,:,-1] is the untouched, all-zero last history slot
                L["ret"] = torch.where(conv, torch.full_like(L["ret"], kk - 1), L["ret"])
                sv.status |= conv.to(torch.int32) * _lib.ST_CONVERGED
                g_conv[gidx[conv[:n]]] = True
                g_status[gidx[conv[:n]]] = sv.status[:n][conv[:n]]  # events up to the stopping iteration
                L["active"] = act = act & ~conv
            if callback is not None:
                callback(kk, sc)
            n_act = int(act.sum())
            if verbose:
                print("Iter = %d\t in flight = %d\t still iterating = %d" % (kk, n, n_act))
            if n_act == 0:
                break
            if compact and n > compact_min and n_act < compact_below * n and kk < prm.max_iters - 2:
                keep = torch.nonzero(act[:n]).squeeze(1)
                flush(sv, gidx, L)
                sv, gidx = sv._compacted(keep), gidx[keep]
                L = fresh(sv)
        flush(sv, gidx, L, final_kk=last)
        return dict(xx_star=out_x.cpu().numpy(), uu_star=out_u.cpu().numpy(), iters=g_iters.cpu().numpy(),
                    converged=g_conv.cpu().numpy(), status=g_status.cpu().numpy(),
                    history={k_: np.stack(v, 1) if v else np.zeros((B, 0)) for k_, v in hist.items()},
                    last_kk=last)

    def solve_on_device(self, sync_every=4, history=True, x_star_f64=False, to_host=True, two_streams=True):
        """solve() through aoc_newton_solve2: the whole loop, stopping rule and return-index bookkeeping on
        the device; the host only reads the count of still-iterating trajectories (every `sync_every` iterations
        while nobody has stopped, more often afterwards; 0: never, all max_iters-1 iterations run) to stop launching
        and to re-pack the iterating trajectories into denser generations.  two_streams: large batches (aoc_tuning.
        solve_split_tiles) are cut in two halves on two HIP streams that never wait for each other.
        Same return value as solve(); results are identical to solve(compact=False).
        to_host=False leaves xx_star (B,6,T) / uu_star (B,2,T) on the device as torch tensors (copying 65 536
        trajectories to the host takes longer than solving them)."""
        torch = _torch()
        B, T, prm, dev = self.B, self.T, self.params, self.problem.device
        n_it = max(int(prm.max_iters) - 1, 0)
        x, f32 = self._xin()
        p = self._p(f32, 0 if x_star_f64 else 1)   # x_star as fp64 or float32 (the same values for iterates >= 1)
        ws = torch.empty((lib().aoc_solve_workspace_bytes(B, T) + 7) // 8, dtype=torch.float64, device=dev)
        x_star = alloc_tiled(B, T, 6, dev, f32=not x_star_f64)
        u_star = torch.zeros_like(self.ub[0])
        iters = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        ret = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        status = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        hf = lambda dt: torch.empty((max(n_it, 1), self.Bp), dtype=dt, device=dev) if history else None
        hc, hd, hs, hn = hf(torch.float64), hf(torch.float64), hf(torch.float64), hf(torch.int32)
        n_run = C.c_int32(0)
        st2 = None
        if two_streams:   # a stream that runs beside the CURRENT one (the pairing is checked once per current stream)
            cur = torch.cuda.current_stream(dev)
            pairs = self.__dict__.setdefault("_stream2_for", {})
            if cur.cuda_stream not in pairs:
                pairs[cur.cuda_stream] = concurrent_streams(dev, 2, first=cur)[1]
            st2 = C.c_void_p(pairs[cur.cuda_stream].cuda_stream)
        torch.cuda.synchronize(dev)
        t_start = time.perf_counter()
        check(lib().aoc_newton_solve2(C.byref(p), C.byref(prm), _ptr(x), _ptr(self.ub[self.cur]), _ptr(self.x0), _ptr(ws), ws.numel() * 8,
                                      int(sync_every), _ptr(x_star), _ptr(u_star), _ptr(iters), _ptr(ret), _ptr(status),
                                      _ptr(hc), _ptr(hd), _ptr(hs), _ptr(hn), C.byref(n_run), st2), "aoc_newton_solve2")
        torch.cuda.synchronize(dev)
        t_device = time.perf_counter() - t_start   # the solve itself; the rest is unpacking and the copy to the host
        del ws
        r = ret[:B]
        xs, us = unpack(x_star, B), unpack(u_star, B)
        xs[:, :, 0] = torch.where((r >= 0)[:, None], unpack_vec(self.x0, B), xs[:, :, 0])  # sample 0 is the fp64 x0
        if self.x_init is not None:  # index 0 is the caller's initial iterate, verbatim
            is0 = r == 0
            xs = torch.where(is0[:, None, None], self.x_init, xs)
            us = torch.where(is0[:, None, None], self.u_init, us)
            us[:, :, -1] = torch.where(is0[:, None], us[:, :, -2], us[:, :, -1])  # optcon.py:505
        st = status[:B].cpu().numpy()
        n = int(n_run.value)
        hist = {}
        for key, h in (("cost", hc), ("descent", hd), ("stepsize", hs), ("ntrials", hn)):
            hist[key] = h[:n, :B].T.cpu().numpy() if history else np.zeros((B, 0))
        return dict(xx_star=xs.cpu().numpy() if to_host else xs, uu_star=us.cpu().numpy() if to_host else us,
                    iters=iters[:B].cpu().numpy(), converged=(st & _lib.ST_CONVERGED) != 0, status=st, history=hist,
                    last_kk=n - 1, device_seconds=t_device)


def solver_arena_bytes(B, T, gran=1 << 21, chunk=None):
    """Bytes an arena must have for one NewtonBatchSolver(B, T) (seven buffers, each rounded up to a handle boundary)."""
    a = chunk or gran
    up = lambda v: (int(v) + a - 1) // a * a
    nt = ntiles(B)
    return (up(lib().aoc_workspace_bytes(B, T) + 8) + 3 * up(nt * T * 6 * TILE * 4) + 3 * up(nt * T * 2 * TILE * 8) + a)


class GradientBatchSolver(NewtonBatchSolver):
    """B independent GradientMethod.optimize instances (reference optcon.py:27-174): steepest descent,
    du = -(B^T lambda + l_u) from the costate sweep (aoc_gradient), Armijo back-tracking and update through the same
    line search as the Newton iteration (aoc_linesearch with no speculated trials).  The reference's own method cannot
    run (TypeError at optcon.py:125); this is its loop with the missing JP argument supplied, pinned to the reference
    run that way (G11: cost, direction and, given the reference's slope, every Armijo verdict and new state; DESIGN
    section 2).  `descent` holds the slope -sum |du|^2 (the reference prints
    +sum |du|^2 and stops when that is <= 1e-6: the same test as slope >= term_cond = -1e-6, so solve() applies
    unchanged, return-index behaviour included)."""

    def iterate(self, kk=None):
        if kk is None:
            kk = self.kk
        x, f32 = self._xin()
        p = self._p(f32)
        c, n = self.cur, (self.cur + 1) % 3
        jc, jn = self.jcur, 1 - self.jcur
        _, du, _, scratch, sbytes, _, _, _ = self._carve()
        check(lib().aoc_gradient(C.byref(p), _ptr(x), _ptr(self.ub[c]), _ptr(self.x0), _ptr(du), _ptr(self.descent),
                                 _ptr(self.status)), "aoc_gradient")
        check(lib().aoc_linesearch(C.byref(p), C.byref(self.params), 0, _ptr(self.ub[c]), _ptr(self.x0), _ptr(du),
                                   _ptr(self.J[jc]), _ptr(self.descent), None, _ptr(self.xb[n]), _ptr(self.ub[n]),
                                   _ptr(self.J[jn]), _ptr(self.stepsize), _ptr(self.ntrials), _ptr(self.status),
                                   _ptr(scratch), sbytes, None, 0), "aoc_linesearch")
        self.cur, self.jcur, self.kk, self.cur_is64, self.cur_rollout = n, jn, kk + 1, False, True

    def direction(self):
        """du (B,2,T) of the last iteration."""
        nel14 = lib().aoc_tiled_elems(self.B, self.T, 14)
        nel2 = lib().aoc_tiled_elems(self.B, self.T, 2)
        return unpack(self.ws[nel14:nel14 + nel2].view(self.nt, self.T, 2, TILE), self.B).cpu().numpy()

    def solve_on_device(self, *a, **kw):
        raise NotImplementedError("aoc_newton_solve runs the Newton iteration; use solve()")


def concurrent_streams(device, n=2, first=None, attempts=16):
    """n HIP streams that really run side by side.  The runtime maps streams onto a few hardware queues (four by default)
    and streams that share a queue take turns: of eight streams created one after the other {2, 3, 7}, {0, 5} and {1, 4}
    shared one, and a two-stream solver on such a pair runs at one-stream speed (5.7 instead of 4.6-4.95 ms per
    iteration: the "second candidate is always the slowest" of the placement probes of round 3 was this).  New streams
    are created until n of them are pairwise concurrent (aoc_streams_concurrent: a 0.2 ms kernel on each).  `first`: a
    stream that must be among them (e.g. the caller's current stream).  Falls back to what it has after `attempts`."""
    torch = _torch()
    dev = torch.device(device)
    good = [first] if first is not None else []
    spare = []
    with torch.cuda.device(dev):      # the probe's events are created on the current device: the streams' device
        for _ in range(attempts):
            if len(good) >= n:
                break
            st = torch.cuda.Stream(device=dev)
            verdicts = [lib().aoc_streams_concurrent(C.c_void_p(g.cuda_stream), C.c_void_p(st.cuda_stream)) for g in good]
            for v in verdicts:
                if v < 0:
                    check(v, "aoc_streams_concurrent")
            (good if all(v == 1 for v in verdicts) else spare).append(st)
        while len(good) < n:      # not enough distinct queues: take what there is
            good.append(spare.pop() if spare else torch.cuda.Stream(device=dev))
    return good


class TwoStreamNewtonSolver:
    """Fixed-iteration runs of a large batch as two half batches on two HIP streams, each a NewtonBatchSolver of its
    own: every kernel takes its stream from aoc_problem, so nothing in the library changes — the halves simply never
    wait for each other.  While one half sits in its latency-bound line-search rounds the other streams through HBM
    (measured, 131 072 trajectories, T = 500: 5.87 -> 5.36 ms per iteration; cutting the batch in two INSIDE one call,
    with a join at the end of every iteration, was slower than one stream: half-size launches only pay while the other
    half keeps the rest of the chip busy).  Per-trajectory results do not depend on the batch a trajectory is solved
    in, so they equal those of one NewtonBatchSolver bit for bit.
    Interface: set_initial_from_x0 / iterate / run_fixed / join / scalars / current / summary_tensors."""

    def __init__(self, problem, B, params=None, streams=None, arenas=None):
        torch = _torch()
        nt = ntiles(B)
        if nt < 2:
            raise ValueError("a batch of one tile cannot be cut in two")
        self.problem, self.B, self.T = problem, int(B), problem.T
        self.Ba = (nt // 2) * TILE
        ar = arenas if arenas is not None else (None, None)      # vmm.Arena per half (see NewtonBatchSolver)
        self.parts = [NewtonBatchSolver(problem, self.Ba, params, arena=ar[0]),
                      NewtonBatchSolver(problem, self.B - self.Ba, params, arena=ar[1])]
        self.params = self.parts[0].params
        # two streams on ONE hardware queue would take turns (concurrent_streams): checked once, here
        self.streams = list(streams) if streams is not None else concurrent_streams(problem.device, len(self.parts))
        self.kk = 0
        self.phased = bool(int(os.environ.get("AOC_TWO_STREAM_PHASED", "0")))   # iterate_phased as the schedule of iterate()
        self._search_done = [None, None]

    def _on(self, fn):
        torch = _torch()
        cur = torch.cuda.current_stream(self.problem.device)
        for i, (sv, st) in enumerate(zip(self.parts, self.streams)):
            st.wait_stream(cur)                      # inputs prepared on the caller's stream are ready
            with torch.cuda.stream(st):
                fn(i, sv)

    def join(self):
        """The caller's stream waits for both halves (before anything reads their results)."""
        torch = _torch()
        cur = torch.cuda.current_stream(self.problem.device)
        for st in self.streams:
            cur.wait_stream(st)

    def set_initial_from_x0(self, x0, kp=5.0, kt=2.5):
        x0 = _dev_f64(x0, self.problem.device)
        cut = (x0[:self.Ba], x0[self.Ba:])
        self._on(lambda i, sv: sv.set_initial_from_x0(cut[i], kp, kt))
        self.kk = 0
        self._search_done = [None, None]
        self.join()

    def iterate(self, kk=None):
        """One outer iteration of every trajectory: enqueued on the two streams, no join (`phased`, off by default:
        see iterate_phased)."""
        if kk is None:
            kk = self.kk
        if self.phased:
            return self.iterate_phased(kk)
        torch = _torch()
        for sv, st in zip(self.parts, self.streams):
            with torch.cuda.stream(st):
                sv.iterate(kk)
        self.kk = kk + 1

    def iterate_phased(self, kk=None):
        """iterate() with the two halves taking turns in their line-search rounds: a half's search waits
        (hipStreamWaitEvent) for the end of the other half's previous search, so the order on the device is A0 B0 A1
        B1 ... and every search runs beside the other half's update / backward / forward passes, never beside its
        search (left to themselves only 40-60 % of a half's search time lies beside a streaming pass of the other one,
        profiles/r05_head_overlap_two_streams.json).  Scheduling only: the same four entry points per half and iteration
        as aoc_newton_iterate issues, results identical (tests/test_gpu_multirank.py).  MEASURED SLOWER and therefore
        off (AOC_TWO_STREAM_PHASED=1 or .phased turns it on): 5.09 against 5.01 ms per iteration over kk 0..19, 4.73 / 4.58
        over kk 0..9 (tools/phase_probe.py, one set of buffers) — the search is not idle time of the chip that a
        schedule could fill: a half's search takes 0.86-1.26 ms per iteration beside the other half (the whole batch's on one
        stream: 1.05 ms) and the passes beside it stretch (profiles/r05_head_overlap_two_streams.json, r05_sq_counters.txt)
        (EXPERIMENTS.md "Two streams, the search as a token")."""
        if kk is None:
            kk = self.kk
        torch = _torch()
        for i, (sv, st) in enumerate(zip(self.parts, self.streams)):
            def between(j, i=i, st=st):
                if j == 2 and self._search_done[1 - i] is not None:
                    st.wait_event(self._search_done[1 - i])
                elif j == 3:
                    ev = torch.cuda.Event()
                    ev.record(st)
                    self._search_done[i] = ev
            with torch.cuda.stream(st):
                sv.iterate_passes(kk, between)
        self.kk = kk + 1

    def run_fixed(self, n_iters, kk0=None):
        if kk0 is not None:
            self.kk = kk0
        for _ in range(n_iters):
            self.iterate()
        self.join()

    def scalars(self):
        self.join()
        a, b = (sv.scalars() for sv in self.parts)
        return {k: np.concatenate([a[k], b[k]]) for k in a}

    def current(self):
        self.join()
        (xa, ua), (xb, ub) = (sv.current() for sv in self.parts)
        return np.concatenate([xa, xb]), np.concatenate([ua, ub])

    def summary_tensors(self):
        """(cost of the newest iterate, descent, trial count) of every trajectory as device tensors, after a join."""
        torch = _torch()
        self.join()
        cat = lambda f: torch.cat([f(sv)[:sv.B] for sv in self.parts])
        return cat(lambda sv: sv.J[sv.jcur]), cat(lambda sv: sv.descent), cat(lambda sv: sv.ntrials)

    def summary(self, out=None):
        """sharding.SUMMARY_FIELDS of the whole batch on the device (aoc_summary: first half, then the second half
        accumulated), on the caller's stream after a join."""
        self.join()
        out = self.parts[0].summary(out)
        return self.parts[1].summary(out, accumulate=True)


def best_placed(make_solver, x0, candidates=5, probe_iters=6, keep_first=False, force=None):
    """Allocation autotuning for large fixed-iteration runs: build `candidates` solvers (make_solver() -> a
    NewtonBatchSolver or TwoStreamNewtonSolver, each with allocations of its own), time Newton iterations
    kk = 0..probe_iters-1 from x0 (B,6) on each, keep the fastest and free the others.

    Why: on MI355X the duration of the write-heavy passes depends on which physical pages hold their output buffers —
    per launch of the backward pass the L2's write requests stall 4-5 times longer for DRAM credits on a "slow"
    allocation, for the same bytes (profiles/r03_placement_pmc.txt) — and the effect is a property of the allocation,
    stable for its lifetime: five two-stream solvers built one after the other in one process run the same 20
    iterations in 4.96, 5.07, 5.47, 5.51 and 6.15 ms each, every time (tools/two_stream_lottery.py).  All candidates
    stay alive until the choice is made (a freed block would simply be handed out again).  Results do not depend on
    the choice: the buffers hold the same values wherever they are.
    Returns (solver, info) with info = {"ms_per_iteration": [...], "chosen": index, "probe_iterations", "probe_wall_s":
    what the choice cost}.  keep_first: candidate 0 — the allocation a caller who does not choose gets — stays alive
    too and is returned as info["first"] (the chosen solver itself when that is candidate 0), so that it can be timed on
    the same workload.  force (tests): take candidate `force % candidates` whatever the probe says."""
    torch = _torch()
    t_wall = time.perf_counter()
    if int(candidates) <= 1:          # nothing to choose from: no probe either
        sv = make_solver()
        info = {"ms_per_iteration": [], "chosen": 0, "probe_iterations": 0, "probe_wall_s": 0.0}
        if keep_first:
            info["first"] = sv
        return sv, info
    cands, ms = [], []
    for _ in range(int(candidates)):
        sv = make_solver()
        dev = sv.problem.device
        xd = _dev_f64(x0, dev)
        best = None
        for rep in range(2):                      # the first pass also warms up lazily loaded code objects
            sv.set_initial_from_x0(xd)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for kk in range(probe_iters):
                sv.iterate(kk)
            sv.join()
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) / probe_iters * 1e3
            best = dt if best is None else min(best, dt)
        cands.append(sv)
        ms.append(round(best, 3))
    chosen = int(np.argmin(ms)) if force is None else int(force) % len(cands)
    keep, first = cands[chosen], cands[0]
    del cands, sv
    info = {"ms_per_iteration": ms, "chosen": chosen, "probe_iterations": probe_iters}
    if keep_first:
        info["first"] = first
    del first
    torch.cuda.empty_cache()
    info["probe_wall_s"] = round(time.perf_counter() - t_wall, 3)
    return keep, info


def traj_cost(problem, xx, uu):
    """Cost of stored trajectories (reference optcon.py:417-424).  xx (B,6,T), uu (B,2,T) -> (B,)"""
    torch = _torch()
    xx = np.asarray(xx, dtype=np.float64)
    xt, ut = pack(xx, problem.device), pack(uu, problem.device)
    B = xx.shape[0]
    x0t = pack_vec(xx[:, :, 0], problem.device)
    J = torch.empty(ntiles(B) * TILE, dtype=torch.float64, device=problem.device)
    p = problem.c_problem(B)
    check(lib().aoc_traj_cost(C.byref(p), _ptr(xt), _ptr(ut), _ptr(x0t), _ptr(J)), "aoc_traj_cost")
    return J[:B].cpu().numpy()


def rollout_cost(problem, x0, uu, du=None, alpha=None, write=True, f32=False):
    """get_update + trial cost (reference optcon.py:176-200, :250-264).
    x0 (B,6), uu (B,2,T), du (B,2,T) or None, alpha (B,) -> (xx (B,6,T), uu' (B,2,T), J (B,), status).
    f32: store the state trajectory as float32 on the device (same values)."""
    torch = _torch()
    dev = problem.device
    B = uu.shape[0]
    ut = pack(uu, dev)
    dt_ = None if du is None else pack(du, dev)
    x0t = pack_vec(x0, dev)
    nt = ntiles(B)
    al = None
    if du is not None:
        al = torch.zeros(nt * TILE, dtype=torch.float64, device=dev)
        al[:B] = _dev_f64(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (B,)).copy(), dev)
    xo = alloc_tiled(B, problem.T, 6, dev, f32=f32) if write else None
    uo = alloc_tiled(B, problem.T, 2, dev) if write else None
    J = torch.empty(nt * TILE, dtype=torch.float64, device=dev)
    st = torch.zeros(nt * TILE, dtype=torch.int32, device=dev)
    p = problem.c_problem(B, x_out_f32=int(f32))
    check(lib().aoc_rollout_cost(C.byref(p), _ptr(x0t), _ptr(ut), _ptr(dt_), _ptr(al), _ptr(xo), _ptr(uo), _ptr(J),
                                 _ptr(st)), "aoc_rollout_cost")
    xx = un = None
    if write:
        xd = unpack(xo, B)
        xd[:, :, 0] = _dev_f64(x0, dev)
        xx, un = xd.cpu().numpy(), unpack(uo, B).cpu().numpy()
    return xx, un, J[:B].cpu().numpy(), st[:B].cpu().numpy()


def backward_forward(problem, xx, uu, full_hessian, stepsize_0=1.0, f32=False):
    """One backward + forward pass (reference optcon.py:429-477 and the first Armijo trial).
    Returns dict with K~ (B,2,7,T), du (B,2,T), descent (B,), lmbd0 (B,6), J_trial0, status.
    f32: hand the state trajectory over as float32 (requires float32-valued samples t >= 1)."""
    torch = _torch()
    dev = problem.device
    xx = np.asarray(xx, dtype=np.float64)
    B, T = xx.shape[0], problem.T
    nt = ntiles(B)
    xt, ut = pack(xx, dev, f32=f32), pack(uu, dev)
    Kt = alloc_tiled(B, T, 14, dev, zero=True)
    du = alloc_tiled(B, T, 2, dev)
    lm0 = torch.empty((nt, 6, TILE), dtype=torch.float64, device=dev)
    desc = torch.empty(nt * TILE, dtype=torch.float64, device=dev)
    Jn = torch.empty(nt * TILE, dtype=torch.float64, device=dev)
    st = torch.zeros(nt * TILE, dtype=torch.int32, device=dev)
    x0t = pack_vec(xx[:, :, 0], dev)
    p = problem.c_problem(B, x_in_f32=int(f32))
    check(lib().aoc_backward(C.byref(p), int(bool(full_hessian)), _ptr(xt), _ptr(ut), _ptr(x0t), _ptr(Kt),
                             _ptr(lm0), _ptr(st), None, 0), "aoc_backward")
    prm = make_params(stepsize_0=stepsize_0)
    check(lib().aoc_forward(C.byref(p), C.byref(prm), 1, _ptr(xt), _ptr(ut), _ptr(x0t), _ptr(Kt), _ptr(du),
                            _ptr(desc), _ptr(Jn), _ptr(st), None, 0, None), "aoc_forward")
    KK = unpack_gains(Kt, B).cpu().numpy()
    return dict(KK=KK, du=unpack(du, B).cpu().numpy(),
                descent=desc[:B].cpu().numpy(), lmbd0=unpack_vec(lm0, B).cpu().numpy(),
                J_trial0=Jn[:B].cpu().numpy(), status=st[:B].cpu().numpy())


def lqr_tracking_batch(problem, xx_opt, uu_opt, delta):
    """lqr_tracking.lqr_tracking for B trajectories (reference lqr_tracking.py:245-283).
    problem carries the tracking weights QQt,RRt,QQT (reference lqr_tracking.py:324-328).
    xx_opt (B,6,T), uu_opt (B,2,T), delta (6,) or (B,6) -> xx_reg (B,6,T), uu_reg (B,2,T), KK (B,2,6,T)."""
    torch = _torch()
    dev = problem.device
    xx_opt = np.asarray(xx_opt, dtype=np.float64)
    B, T = xx_opt.shape[0], problem.T
    nt = ntiles(B)
    xt, ut = pack(xx_opt, dev), pack(uu_opt, dev)
    x0r = xx_opt[:, :, 0] + np.broadcast_to(np.asarray(delta, dtype=np.float64), (B, 6))  # lqr_tracking.py:265
    x0t = pack_vec(x0r, dev)
    xo0 = pack_vec(xx_opt[:, :, 0], dev)
    Kg = alloc_tiled(B, T, 12, dev)
    xr, ur = alloc_tiled(B, T, 6, dev), alloc_tiled(B, T, 2, dev)
    st = torch.zeros(nt * TILE, dtype=torch.int32, device=dev)
    p = problem.c_problem(B)
    check(lib().aoc_lqr_tracking(C.byref(p), _ptr(xt), _ptr(ut), _ptr(xo0), _ptr(x0t), _ptr(Kg), _ptr(xr), _ptr(ur),
                                 _ptr(st)), "aoc_lqr_tracking")
    KK = unpack(Kg, B).cpu().numpy().reshape(B, 2, 6, T)
    return unpack(xr, B).cpu().numpy(), unpack(ur, B).cpu().numpy(), KK, st[:B].cpu().numpy()


# ------------------------------------------------------------------------------------------------
# closed-loop tracking ensembles about shared optima (aoc_track_ensemble)
# ------------------------------------------------------------------------------------------------
ENS_REC = 20                       # doubles per stage record of `nominal`
ENS_NSTAT = _lib.AOC_ENS_NSTAT     # statistics per member
ENS_QUANTILES = (0.5, 0.9, 0.99)
ENV_NREC = _lib.AOC_ENV_NREC       # doubles per (optimum, sample) record of aoc_track_ensemble_envelope
HIST_NCH = _lib.AOC_HIST_NCH       # channels of aoc_track_ensemble_histogram: dx[0..5], du[0..1]
HIST_NBIN = _lib.AOC_HIST_NBIN     # bins per (optimum, sample, channel)
COV_NREC = _lib.AOC_COV_NREC       # doubles per (optimum, sample) record of aoc_track_covariance
SAT_NSTAT = _lib.AOC_SAT_NSTAT     # cut statistics per member of aoc_track_ensemble_limited
LQG_NSTAT = _lib.AOC_LQG_NSTAT     # estimation-error statistics per member of aoc_track_ensemble_lqg
FILT_NREC = _lib.AOC_FILT_NREC     # doubles per (optimum, sample) covariance record of aoc_filter_gains
LQGCOV_NREC = _lib.AOC_LQGCOV_NREC # doubles per (optimum, sample) record of aoc_track_covariance_lqg
# the record (include/aoc.h): n | min dx | max dx | min du | max du | sum dx | sum dx_i dx_j (upper triangle, row by row)
_ENV_MIN = np.r_[1:7, 13:15]
_ENV_MAX = np.r_[7:13, 15:17]
_ENV_SUM = np.r_[0:1, 17:44]
_ENV_TRI = np.triu_indices(6)


def ensemble_nominal(xx_opt, uu_opt, KK):
    """The `nominal` array of aoc_track_ensemble on the host: xx_opt (n_opt,6,T), uu_opt (n_opt,2,T), KK (n_opt,2,6,T)
    -> (n_opt,T,20) fp64, per sample x_opt[0..5], u_opt[0..1], K row 0 [0..5], K row 1 [0..5].  Needs no GPU."""
    xo, uo, K = (np.asarray(a, dtype=np.float64) for a in (xx_opt, uu_opt, KK))
    n, _, T = xo.shape
    if xo.shape != (n, 6, T) or uo.shape != (n, 2, T) or K.shape != (n, 2, 6, T):
        raise ValueError("xx_opt (n_opt,6,T), uu_opt (n_opt,2,T), KK (n_opt,2,6,T) expected, got %s %s %s"
                         % (xo.shape, uo.shape, K.shape))
    return np.ascontiguousarray(np.concatenate([xo, uo, K.reshape(n, 12, T)], axis=1).transpose(0, 2, 1))


def ensemble_groups(B, n_opt, members_per_opt=None):
    """How B members are dealt to n_opt optima: whole tiles, member b belongs to optimum b // members_per_opt.
    members_per_opt=None: B spread evenly, rounded up to whole tiles.  -> (members_per_opt, group (B,) int).  Raises
    ValueError where aoc_track_ensemble would refuse the geometry.  Needs no GPU."""
    B, n_opt = int(B), int(n_opt)
    if B < 1 or n_opt < 1:
        raise ValueError("B = %d members, n_opt = %d optima" % (B, n_opt))
    mpo = -(-(-(-B // n_opt)) // TILE) * TILE if members_per_opt is None else int(members_per_opt)
    if mpo < TILE or mpo % TILE:
        raise ValueError("members_per_opt = %d is not a positive multiple of %d" % (mpo, TILE))
    if not (n_opt - 1) * mpo < B <= n_opt * mpo:
        raise ValueError("B = %d members do not fill %d groups of %d (the last group may be partial, none empty)"
                         % (B, n_opt, mpo))
    return mpo, np.arange(B) // mpo


def tracking_gains(problem, xx_opt, uu_opt):
    """Tracking gains only (lqr_tracking.py:268-276) about n optima: ONE aoc_lqr_tracking call without the rollout.
    xx_opt (n,6,T), uu_opt (n,2,T) -> KK (n,2,6,T) numpy, status (n,)."""
    torch = _torch()
    dev = problem.device
    xx_opt = np.asarray(xx_opt, dtype=np.float64)
    n, T = xx_opt.shape[0], problem.T
    xt, ut = pack(xx_opt, dev), pack(uu_opt, dev)
    xo0 = pack_vec(xx_opt[:, :, 0], dev)
    Kg = alloc_tiled(n, T, 12, dev)
    st = torch.zeros(ntiles(n) * TILE, dtype=torch.int32, device=dev)
    p = problem.c_problem(n)
    check(lib().aoc_lqr_tracking(C.byref(p), _ptr(xt), _ptr(ut), _ptr(xo0), None, _ptr(Kg), None, None, _ptr(st)),
          "aoc_lqr_tracking")
    return unpack(Kg, n).cpu().numpy().reshape(n, 2, 6, T), st[:n].cpu().numpy()


def envelope_merge(raw_a, raw_b):
    """Records (..., 44) of two disjoint sets of members of the same optimum -> the record of their union: n and the sums
    add, the minima and maxima combine.  What joins calls cut by `first=`, and what a multi-GPU job all-reduces (SUM for
    0 and 17-43, MIN for 1-6 and 13-14, MAX for 7-12 and 15-16).  NumPy only, needs no GPU."""
    a, b = np.asarray(raw_a, dtype=np.float64), np.asarray(raw_b, dtype=np.float64)
    if a.shape != b.shape or a.shape[-1] != ENV_NREC:
        raise ValueError("two arrays of records (..., %d) of one shape expected, got %s %s" % (ENV_NREC, a.shape, b.shape))
    out = np.empty_like(a)
    out[..., _ENV_SUM] = a[..., _ENV_SUM] + b[..., _ENV_SUM]
    out[..., _ENV_MIN] = np.minimum(a[..., _ENV_MIN], b[..., _ENV_MIN])
    out[..., _ENV_MAX] = np.maximum(a[..., _ENV_MAX], b[..., _ENV_MAX])
    return out


def envelope_moments(raw):
    """Records (T, 44) -> n (T,) int, mean_dx (6,T), cov_dx (6,6,T): the population covariance E[dx dx^T] - E[dx] E[dx]^T
    from the raw moments; mean and covariance are NaN where n = 0.  NumPy only, needs no GPU."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 2 or raw.shape[1] != ENV_NREC:
        raise ValueError("records (T, %d) expected, got %s" % (ENV_NREC, raw.shape))
    n = raw[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n[:, None] > 0, raw[:, 17:23] / n[:, None], np.nan)           # (T,6)
        second = np.empty((raw.shape[0], 6, 6))
        second[:, _ENV_TRI[0], _ENV_TRI[1]] = raw[:, 23:44]
        second[:, _ENV_TRI[1], _ENV_TRI[0]] = raw[:, 23:44]
        second = np.where(n[:, None, None] > 0, second / n[:, None, None], np.nan)
    cov = second - mean[:, :, None] * mean[:, None, :]
    return n.astype(np.int64), np.ascontiguousarray(mean.T), np.ascontiguousarray(cov.transpose(1, 2, 0))


def _envelope_dict(raw):
    n, mean, cov = envelope_moments(raw)
    return dict(n=n, min_dx=raw[:, 1:7].T.copy(), max_dx=raw[:, 7:13].T.copy(), min_du=raw[:, 13:15].T.copy(),
                max_du=raw[:, 15:17].T.copy(), mean_dx=mean, cov_dx=cov, raw=raw)


def histogram_bins(envelope_raw, pad=0.0):
    """Equal bins over what the envelope saw: records (n_opt,T,44) (or (T,44)) -> bins (n_opt,T,8,2) = (lo, inv_w) per
    optimum, sample and channel (dx[0..5], du[0..1]), the `bins` of aoc_track_ensemble_histogram: lo = min, inv_w =
    64 / (max - min), the range widened by pad * (max - min) on either side first.  Where max == min the bins are
    (that value, 0), where n = 0 (min / max infinite; du at sample T-1) they are (0, 0): everything then goes to bin 0.
    NumPy only, needs no GPU."""
    raw = np.asarray(envelope_raw, dtype=np.float64)
    raw = raw[None] if raw.ndim == 2 else raw
    if raw.ndim != 3 or raw.shape[2] != ENV_NREC:
        raise ValueError("records (n_opt, T, %d) expected, got %s" % (ENV_NREC, raw.shape))
    mn, mx = raw[..., _ENV_MIN], raw[..., _ENV_MAX]
    some = np.isfinite(mn) & np.isfinite(mx)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        span = np.where(some, mx - mn, 0.0)
        lo = np.where(some, mn - pad * span, 0.0)
        w = span * (1.0 + 2.0 * pad)
        inv_w = np.where(some & (w > 0) & np.isfinite(w), HIST_NBIN / w, 0.0)
    inv_w = np.where(np.isfinite(inv_w), inv_w, 0.0)          # a range so narrow that 64 / w overflows: one value
    return np.ascontiguousarray(np.stack([lo, inv_w], axis=-1))


def histogram_merge(a, b):
    """Counts (..., 8, 64) of two disjoint sets of members under the SAME bins -> the counts of their union: addition.
    What joins calls cut by `first=`, shards and devices.  NumPy only, needs no GPU."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.shape[-2:] != (HIST_NCH, HIST_NBIN) or a.dtype.kind not in "iu" or b.dtype.kind not in "iu":
        raise ValueError("two integer arrays of counts (..., %d, %d) of one shape expected, got %s %s %s %s"
                         % (HIST_NCH, HIST_NBIN, a.shape, a.dtype, b.shape, b.dtype))
    return a.astype(np.int64) + b.astype(np.int64)


def sat_count_merge(a, b):
    """Cut counts (..., T, 2) of two disjoint sets of members of the same optimum under the SAME limits -> the counts of
    their union: addition.  What joins calls cut by `first=`, shards and devices.  NumPy only, needs no GPU."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim < 2 or a.shape[-1] != 2 or a.dtype.kind not in "iu" or b.dtype.kind not in "iu":
        raise ValueError("two integer arrays of counts (..., T, 2) of one shape expected, got %s %s %s %s"
                         % (a.shape, a.dtype, b.shape, b.dtype))
    return a.astype(np.int64) + b.astype(np.int64)


def frac_cut(sat):
    """sat (M, 6) of some members -> (2,): per channel the share of them that is cut at least once (sat[:, 0:2] > 0; a
    member whose demand is NaN throughout is never cut).  NaN for no members.  NumPy only, needs no GPU."""
    sat = np.asarray(sat, dtype=np.float64)
    if sat.ndim != 2 or sat.shape[1] != SAT_NSTAT:
        raise ValueError("cut statistics (M, %d) expected, got %s" % (SAT_NSTAT, sat.shape))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (sat[:, 0:2] > 0).sum(axis=0) / np.float64(sat.shape[0])


def actuator_limits(u_min=None, u_max=None, u_rate=None):
    """The three keywords of track_ensemble -> lo, hi, rate (2,) fp64 with None (the keyword or a component) = unbounded;
    ValueError for a shape other than (2,), a NaN, lo > hi or rate <= 0 — what aoc_track_ensemble_limited refuses."""
    def two(v, default, name):
        if v is None:
            return np.full(2, default)
        a = np.array([default if c is None else c for c in v] if np.ndim(v) == 1 else v, dtype=np.float64)
        if a.shape != (2,) or np.isnan(a).any():
            raise ValueError("%s must be (2,) = (thrust, pitching moment) without NaN, got %r" % (name, v))
        return a
    lo, hi, rate = two(u_min, -np.inf, "u_min"), two(u_max, np.inf, "u_max"), two(u_rate, np.inf, "u_rate")
    if (lo > hi).any():
        raise ValueError("u_min = %s exceeds u_max = %s" % (lo, hi))
    if (rate <= 0).any():
        raise ValueError("u_rate = %s must be positive (None or inf: no rate limit)" % (rate,))
    return lo, hi, rate


def histogram_quantiles(hist, bins, q):
    """Quantile tubes from counts: hist (n_opt,T,8,64) (or (T,8,64)), bins (n_opt,T,8,2) (or (T,8,2)), q a sequence of
    levels in [0,1] -> tube (len(q),n_opt,8,T), width (n_opt,8,T).  With n the sum of the counts of (optimum, sample,
    channel) and r = max(1, ceil(q n)), the value is the midpoint lo + (k + 0.5) / inv_w of the first bin k whose
    cumulative count reaches r (lo where inv_w = 0), NaN where n = 0; width = 1 / inv_w (0 where inv_w = 0) is the
    resolution: where nothing fell outside the bins, the r-th order statistic lies in bin k, within width / 2 of the
    value.  NumPy only, needs no GPU."""
    h, b = np.asarray(hist), np.asarray(bins, dtype=np.float64)
    if h.ndim == 3:
        h, b = h[None], (b[None] if b.ndim == 3 else b)
    if h.ndim != 4 or h.shape[2:] != (HIST_NCH, HIST_NBIN) or b.shape != h.shape[:3] + (2,):
        raise ValueError("hist (n_opt,T,%d,%d) and bins (n_opt,T,%d,2) expected, got %s %s"
                         % (HIST_NCH, HIST_NBIN, HIST_NCH, h.shape, b.shape))
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not np.all((q >= 0) & (q <= 1)):
        raise ValueError("quantile levels in [0, 1] expected, got %s" % (q,))
    cum = np.cumsum(h.astype(np.int64), axis=-1)                                  # (n_opt,T,8,64)
    n = cum[..., -1]
    lo, inv_w = b[..., 0], b[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        width = np.where(inv_w != 0, 1.0 / inv_w, 0.0)
    tube = np.empty((q.size,) + n.shape)
    for i, f in enumerate(q):
        r = np.maximum(1, np.ceil(f * n)).astype(np.int64)
        k = (cum < r[..., None]).sum(axis=-1)                                     # first bin whose cumulative count reaches r
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.where(inv_w != 0, lo + (k + 0.5) / inv_w, lo)
        tube[i] = np.where(n > 0, mid, np.nan)
    return np.ascontiguousarray(tube.transpose(0, 1, 3, 2)), np.ascontiguousarray(width.transpose(0, 2, 1))


def covariance_moments(raw):
    """Records (T, 32) of aoc_track_covariance -> mean_dx (6,T), cov_dx (6,6,T), mean_du (2,T), cov_du (2,2,T): what linear
    theory predicts for dx = x - x_opt and du = u - u_opt (sample T-1 of the input moments is 0: there is no input).
    NumPy only, needs no GPU."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 2 or raw.shape[1] != COV_NREC:
        raise ValueError("records (T, %d) expected, got %s" % (COV_NREC, raw.shape))
    T = raw.shape[0]
    cov = np.empty((T, 6, 6))
    cov[:, _ENV_TRI[0], _ENV_TRI[1]] = raw[:, 6:27]
    cov[:, _ENV_TRI[1], _ENV_TRI[0]] = raw[:, 6:27]
    cu = np.empty((T, 2, 2))
    cu[:, 0, 0], cu[:, 0, 1], cu[:, 1, 0], cu[:, 1, 1] = raw[:, 29], raw[:, 30], raw[:, 30], raw[:, 31]
    return (np.ascontiguousarray(raw[:, 0:6].T), np.ascontiguousarray(cov.transpose(1, 2, 0)),
            np.ascontiguousarray(raw[:, 27:29].T), np.ascontiguousarray(cu.transpose(1, 2, 0)))


def _covariance_dict(raw):
    mean_dx, cov_dx, mean_du, cov_du = covariance_moments(raw)
    return dict(mean_dx=mean_dx, cov_dx=cov_dx, mean_du=mean_du, cov_du=cov_du, raw=raw)


_COV_MEAN = np.r_[0:6, 27:29]                                                       # the eight channels' means ...
_COV_VAR = np.r_[[6 + int(i * 6 - i * (i - 1) // 2) for i in range(6)], 29, 31]     # ... and variances in a record


def histogram_bins_predicted(raw, k=6.0):
    """Bins from the prediction instead of a first pass: records (n_opt,T,32) (or (T,32)) of aoc_track_covariance -> bins
    (n_opt,T,8,2) = (lo, inv_w) per optimum, sample and channel (dx[0..5], du[0..1]): lo = mean - k std, inv_w =
    64 / (2 k std).  Where std is 0 or not finite (a channel nothing moves; du at sample T-1) the bins are (mean, 0), and
    (0, 0) if the mean is not finite either: everything then goes to bin 0.  NumPy only, needs no GPU."""
    raw = np.asarray(raw, dtype=np.float64)
    raw = raw[None] if raw.ndim == 2 else raw
    if raw.ndim != 3 or raw.shape[2] != COV_NREC:
        raise ValueError("records (n_opt, T, %d) expected, got %s" % (COV_NREC, raw.shape))
    k = float(k)
    if not k > 0:
        raise ValueError("k = %r (need k > 0)" % (k,))
    mean, var = raw[..., _COV_MEAN], raw[..., _COV_VAR]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        std = np.sqrt(var)
        w = 2.0 * k * std
        ok = np.isfinite(mean) & np.isfinite(w) & (w > 0)
        inv_w = np.where(ok, HIST_NBIN / w, 0.0)
        ok &= np.isfinite(inv_w)
        lo = np.where(ok, mean - k * std, np.where(np.isfinite(mean), mean, 0.0))
    return np.ascontiguousarray(np.stack([lo, np.where(ok, inv_w, 0.0)], axis=-1))


def _sym_upper(Sigma0, n_opt):
    """(6,6) or (n_opt,6,6), symmetric (checked) -> (n_opt,21) upper triangle row by row"""
    S = np.asarray(Sigma0, dtype=np.float64)
    S = np.broadcast_to(S, (n_opt, 6, 6)) if S.ndim == 2 else S
    if S.shape != (n_opt, 6, 6):
        raise ValueError("Sigma0 must be (6,6) or (n_opt,6,6) with n_opt = %d, got %s" % (n_opt, S.shape))
    if not np.array_equal(S, S.transpose(0, 2, 1)):
        raise ValueError("Sigma0 is not symmetric")
    return np.ascontiguousarray(S[:, _ENV_TRI[0], _ENV_TRI[1]])


def _predict_covariance(problem, nominal, n_opt, mean0, Sigma0, sigma):
    """aoc_track_covariance on a device `nominal` (n_opt,T,20) -> records (n_opt,T,32) numpy, status (n_opt,)"""
    torch = _torch()
    dev, T = problem.device, problem.T
    m0 = S0 = None
    if mean0 is not None:
        m = np.asarray(mean0, dtype=np.float64)
        m = np.broadcast_to(m, (n_opt, 6)) if m.ndim == 1 else m
        if m.shape != (n_opt, 6):
            raise ValueError("mean0 must be (6,) or (n_opt,6) with n_opt = %d, got %s" % (n_opt, m.shape))
        m0 = _dev_f64(m, dev)
    if Sigma0 is not None:
        S0 = _dev_f64(_sym_upper(Sigma0, n_opt), dev)
    nz = None
    if sigma is not None:
        nz = _lib.MpcNoise(0, 0, 0, (C.c_double * 6)(*np.asarray(sigma, dtype=np.float64).tolist()))
    pred = torch.empty((n_opt, T, COV_NREC), dtype=torch.float64, device=dev)
    status = torch.zeros(n_opt, dtype=torch.int32, device=dev)
    nbytes = int(lib().aoc_track_covariance_scratch_bytes(n_opt, T))
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    p = problem.c_problem(n_opt)
    check(lib().aoc_track_covariance(C.byref(p), n_opt, _ptr(nominal), _ptr(m0), _ptr(S0), C.byref(nz) if nz is not None else None,
                                     _ptr(pred), _ptr(status), _ptr(scratch), nbytes), "aoc_track_covariance")
    return pred.cpu().numpy(), status.cpu().numpy()


def predict_covariance(problem, xx_opt, uu_opt, KK=None, mean0=None, Sigma0=None, sigma=None):
    """What linear theory predicts for a closed-loop tracking ensemble about each optimum (aoc_track_covariance): the mean
    and covariance of dx = x - x_opt and of du = u - u_opt at every sample, from the Lyapunov recursion with the tracking
    gains, m' = F m + c, P' = F P F^T + diag(sigma^2), F = A + B K (include/aoc.h).  xx_opt (6,T) or (n_opt,6,T), uu_opt
    likewise; KK=None: gains from tracking_gains; mean0 (6,) or (n_opt,6) and Sigma0 (6,6) or (n_opt,6,6) (symmetric,
    checked here) are the moments of dx at sample 0, None = 0; sigma (6,) the std of the disturbance, None = none.
    Returns (list per optimum of dict(mean_dx (6,T), cov_dx (6,6,T), mean_du (2,T), cov_du (2,2,T), raw (T,32)),
    status (n_opt,))."""
    torch = _torch()
    xo, uo = np.asarray(xx_opt, dtype=np.float64), np.asarray(uu_opt, dtype=np.float64)
    if xo.ndim == 2:
        xo, uo = xo[None], uo[None]
    n_opt, T = xo.shape[0], problem.T
    if xo.shape != (n_opt, 6, T) or uo.shape != (n_opt, 2, T):
        raise ValueError("xx_opt must be (6,T) or (n_opt,6,T) with T = %d, uu_opt likewise" % T)
    if KK is None:
        KK, _ = tracking_gains(problem, xo, uo)
    else:
        KK = np.asarray(KK, dtype=np.float64)
        KK = KK[None] if KK.ndim == 3 else KK
    nominal = torch.from_numpy(ensemble_nominal(xo, uo, KK)).to(problem.device)
    raw, status = _predict_covariance(problem, nominal, n_opt, mean0, Sigma0, sigma)
    return [_covariance_dict(r) for r in raw], status


def lqg_covariance_moments(raw):
    """Records (T, 96) of aoc_track_covariance_lqg -> dict(mean_dx (6,T), cov_dx (6,6,T), mean_e (6,T), cov_e (6,6,T),
    cov_dx_e (6,6,T) with [i,j] = cov(dx_i, e_j), cov_xhat (6,6,T) = X - C - C^T + E, the covariance of the estimate e^+
    (formed here), mean_du (2,T), cov_du (2,2,T), raw): what linear theory predicts for the LQG loop, e = dx - e^+ the
    posterior estimation error (sample T-1 of the input moments is 0: there is no input).  NumPy only, needs no GPU."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 2 or raw.shape[1] != LQGCOV_NREC:
        raise ValueError("records (T, %d) expected, got %s" % (LQGCOV_NREC, raw.shape))
    T = raw.shape[0]
    X, E = np.empty((T, 6, 6)), np.empty((T, 6, 6))
    for M, o in ((X, 12), (E, 33)):
        M[:, _ENV_TRI[0], _ENV_TRI[1]] = raw[:, o:o + 21]
        M[:, _ENV_TRI[1], _ENV_TRI[0]] = raw[:, o:o + 21]
    Cx = raw[:, 54:90].reshape(T, 6, 6)
    cu = np.empty((T, 2, 2))
    cu[:, 0, 0], cu[:, 0, 1], cu[:, 1, 0], cu[:, 1, 1] = raw[:, 92], raw[:, 93], raw[:, 93], raw[:, 94]
    tm = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0))
    return dict(mean_dx=np.ascontiguousarray(raw[:, 0:6].T), cov_dx=tm(X), mean_e=np.ascontiguousarray(raw[:, 6:12].T),
                cov_e=tm(E), cov_dx_e=tm(Cx), cov_xhat=tm(X - Cx - Cx.transpose(0, 2, 1) + E),
                mean_du=np.ascontiguousarray(raw[:, 90:92].T), cov_du=tm(cu), raw=raw)


def _rows6(a, n_opt, name):
    """None, (6,) or (n_opt,6) -> (n_opt,6) contiguous, or None"""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    a = np.broadcast_to(a, (n_opt, 6)) if a.ndim == 1 else a
    if a.shape != (n_opt, 6):
        raise ValueError("%s must be (6,) or (n_opt,6) with n_opt = %d, got %s" % (name, n_opt, a.shape))
    return np.ascontiguousarray(a)


def _filter_to_device(filter, n_opt, T, dev):
    """L (6,6,T) or (n_opt,6,6,T) -> the device array [n_opt][T][36] of aoc_track_ensemble_lqg / aoc_track_covariance_lqg"""
    Lf = np.asarray(filter, dtype=np.float64)
    Lf = Lf[None] if Lf.ndim == 3 else Lf
    if Lf.shape != (n_opt, 6, 6, T):
        raise ValueError("filter must be (6,6,T) or (n_opt,6,6,T) = %s, got %s" % ((n_opt, 6, 6, T), Lf.shape))
    return _torch().from_numpy(np.ascontiguousarray(Lf.reshape(n_opt, 36, T).transpose(0, 2, 1))).to(dev)


def _predict_covariance_lqg(problem, nominal, filt_d, n_opt, mean0, ehat0, Sigma0, sigma, rho):
    """aoc_track_covariance_lqg on a device `nominal` (n_opt,T,20) and device gains (n_opt,T,36), on the current stream ->
    records (n_opt,T,96) numpy, status (n_opt,)"""
    torch = _torch()
    dev, T = problem.device, problem.T
    m0, e0 = _rows6(mean0, n_opt, "mean0"), _rows6(ehat0, n_opt, "ehat0")
    m0 = _dev_f64(m0, dev) if m0 is not None else None
    e0 = _dev_f64(e0, dev) if e0 is not None else None
    S0 = _dev_f64(_sym_upper(Sigma0, n_opt), dev) if Sigma0 is not None else None
    nz = None
    if sigma is not None:
        nz = _lib.MpcNoise(0, 0, 0, (C.c_double * 6)(*np.asarray(sigma, dtype=np.float64).reshape(6).tolist()))
    rho_c = None
    if rho is not None:
        rho_c = (C.c_double * 6)(*np.asarray(rho, dtype=np.float64).reshape(6).tolist())
    pred = torch.empty((n_opt, T, LQGCOV_NREC), dtype=torch.float64, device=dev)
    status = torch.zeros(n_opt, dtype=torch.int32, device=dev)
    nbytes = int(lib().aoc_track_covariance_lqg_scratch_bytes(n_opt, T))
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    p = problem.c_problem(n_opt)
    check(lib().aoc_track_covariance_lqg(C.byref(p), n_opt, _ptr(nominal), _ptr(filt_d), _ptr(m0), _ptr(e0), _ptr(S0),
                                         C.byref(nz) if nz is not None else None, rho_c, _ptr(pred), _ptr(status),
                                         _ptr(scratch), nbytes), "aoc_track_covariance_lqg")
    return pred.cpu().numpy(), status.cpu().numpy()


def predict_covariance_lqg(problem, xx_opt, uu_opt, filter, KK=None, mean0=None, ehat0=None, Sigma0=None, sigma=None,
                           rho=None, measured=None):
    """What linear theory predicts for the LQG loop of track_ensemble(filter=) about each optimum (aoc_track_covariance_lqg):
    the joint mean and covariance of dx = x - x_opt and of the posterior estimation error e = dx - e^+ at every sample, and
    the moments of du, for ANY gains L — the recursion of include/aoc.h.  xx_opt (6,T) or (n_opt,6,T), uu_opt likewise;
    filter: L (6,6,T) or (n_opt,6,6,T), or "device": the gains of aoc_filter_gains on the same stream, which do not visit
    the host — Sigma0 (required then), sigma, rho (required then) and `measured` are used as filter_gains_device uses them.
    KK=None: gains from tracking_gains; mean0, ehat0 (6,) or (n_opt,6): the mean of dx_0 and the prior estimate, None = 0;
    Sigma0 (6,6) or (n_opt,6,6), symmetric: the covariance of dx_0 (and of the prior error), None = 0; sigma, rho (6,): the
    std of the disturbance and of the measurement noise, None = 0.
    Returns (list per optimum of lqg_covariance_moments' dict, status (n_opt,))."""
    device_gains = isinstance(filter, str)
    if filter is None:
        raise ValueError("filter= is required: L (6,6,T) or (n_opt,6,6,T), or \"device\"")
    if device_gains:
        if filter != "device":
            raise ValueError('filter=%r: the only name is "device"' % (filter,))
        if Sigma0 is None or rho is None:
            raise ValueError('filter="device" needs Sigma0= (the covariance of the prior estimate\'s error) and rho=')
        mask = _measured_mask(measured)
    elif measured is not None:
        raise ValueError('measured= goes with filter="device"')
    xo, uo = np.asarray(xx_opt, dtype=np.float64), np.asarray(uu_opt, dtype=np.float64)
    if xo.ndim == 2:
        xo, uo = xo[None], uo[None]
    n_opt, T = xo.shape[0], problem.T
    if xo.shape != (n_opt, 6, T) or uo.shape != (n_opt, 2, T):
        raise ValueError("xx_opt must be (6,T) or (n_opt,6,T) with T = %d, uu_opt likewise" % T)
    if not device_gains:
        Lf = np.asarray(filter, dtype=np.float64)
        if (Lf[None] if Lf.ndim == 3 else Lf).shape != (n_opt, 6, 6, T):
            raise ValueError("filter must be (6,6,T) or (n_opt,6,6,T) = %s, got %s" % ((n_opt, 6, 6, T), Lf.shape))
    torch = _torch()
    if KK is None:
        KK, _ = tracking_gains(problem, xo, uo)
    else:
        KK = np.asarray(KK, dtype=np.float64)
        KK = KK[None] if KK.ndim == 3 else KK
    nominal = torch.from_numpy(ensemble_nominal(xo, uo, KK)).to(problem.device)
    if device_gains:
        filt_d, _, _ = _filter_gains_device(problem, nominal, n_opt, Sigma0, sigma, rho, mask, False)
    else:
        filt_d = _filter_to_device(filter, n_opt, T, problem.device)
    raw, status = _predict_covariance_lqg(problem, nominal, filt_d, n_opt, mean0, ehat0, Sigma0, sigma, rho)
    return [lqg_covariance_moments(r) for r in raw], status


def filter_gains(problem, xx_opt, uu_opt, Sigma0, sigma, rho, jac=None):
    """Gains of the Kalman filter linearised about ONE optimum, for track_ensemble(rho=, filter=): the recursion in NumPy,
        L_t = P^-_t (P^-_t + V)^-1,   P^+_t = (I - L_t) P^-_t (I - L_t)^T + L_t V L_t^T   (Joseph form),
        P^-_{t+1} = A_t P^+_t A_t^T + W,      P^-_0 = Sigma0,  W = diag(sigma^2),  V = diag(rho^2),
    for the measurement y = dx + v of the whole deviation.  xx_opt (6,T), uu_opt (2,T); Sigma0 (6,6) the covariance of the
    prior estimate's error at sample 0; sigma (6,) the std of the disturbance (None = 0), rho (6,) that of the measurement
    noise, every component > 0.  A_t (and B_t, unused by a filter that knows its input) are the Jacobians of Dynamics.step
    along the optimum: from step_batch on the device, or jac=(A (T-1,6,6), B (T-1,6,2)) as given (the oracle's, where no
    GPU is at hand).  Returns L (6,6,T), P_prior (6,6,T), P_post (6,6,T)."""
    xo, uo = np.asarray(xx_opt, dtype=np.float64), np.asarray(uu_opt, dtype=np.float64)
    T = xo.shape[1]
    if xo.shape != (6, T) or uo.shape != (2, T):
        raise ValueError("xx_opt (6,T) and uu_opt (2,T) expected, got %s %s" % (xo.shape, uo.shape))
    rho = np.asarray(rho, dtype=np.float64)
    if rho.shape != (6,) or not np.all(np.isfinite(rho) & (rho > 0)):
        raise ValueError("rho must be six finite standard deviations > 0, got %s" % (rho,))
    W = np.zeros((6, 6)) if sigma is None else np.diag(np.asarray(sigma, dtype=np.float64) ** 2)
    V = np.diag(rho ** 2)
    P = np.asarray(Sigma0, dtype=np.float64)
    if P.shape != (6, 6) or not np.array_equal(P, P.T):
        raise ValueError("Sigma0 must be a symmetric (6,6) matrix")
    if jac is None:
        _, fx, _, _, _, _ = step_batch(problem.model, xo[:, :T - 1].T, uo[:, :T - 1].T, device=problem.device)
        A = fx.transpose(0, 2, 1)                                 # aoc_step_batch: fx = A^T
    else:
        A = np.asarray(jac[0], dtype=np.float64)
    if A.shape != (T - 1, 6, 6):
        raise ValueError("A must be (T-1,6,6) = %s, got %s" % ((T - 1, 6, 6), A.shape))
    L, Pm, Pp = np.zeros((6, 6, T)), np.zeros((6, 6, T)), np.zeros((6, 6, T))
    I = np.eye(6)
    for t in range(T):
        Lt = np.linalg.solve(P + V, P).T                          # P (P + V)^-1, both symmetric
        post = (I - Lt) @ P @ (I - Lt).T + Lt @ V @ Lt.T
        post = 0.5 * (post + post.T)
        L[:, :, t], Pm[:, :, t], Pp[:, :, t] = Lt, P, post
        if t < T - 1:
            P = A[t] @ post @ A[t].T + W
            P = 0.5 * (P + P.T)
    return L, Pm, Pp


def _measured_mask(measured):
    """a sequence of channel indices, or None = all six -> the 6-bit mask of aoc_filter_gains"""
    if measured is None:
        return 63
    mask = 0
    for c in measured:
        if int(c) != c or not 0 <= int(c) < 6:
            raise ValueError("measured must be channel indices 0 .. 5 (or None = all), got %r" % (measured,))
        mask |= 1 << int(c)
    return mask


def _filter_gains_device(problem, nominal, n_opt, Sigma0, sigma, rho, mask, want_cov):
    """aoc_filter_gains on a device `nominal` (n_opt,T,20), on the current stream -> device tensors filter (n_opt,T,36),
    cov (n_opt,T,42) or None, status (n_opt,).  The rho rules are the call's own: a refusal is an AocError with its reason."""
    torch = _torch()
    dev, T = problem.device, problem.T
    S0 = _dev_f64(_sym_upper(Sigma0, n_opt), dev)
    nz = None
    if sigma is not None:
        nz = _lib.MpcNoise(0, 0, 0, (C.c_double * 6)(*np.asarray(sigma, dtype=np.float64).reshape(6).tolist()))
    rho_c = (C.c_double * 6)(*np.asarray(rho, dtype=np.float64).reshape(6).tolist())
    filt = torch.empty((n_opt, T, 36), dtype=torch.float64, device=dev)
    cov = torch.empty((n_opt, T, FILT_NREC), dtype=torch.float64, device=dev) if want_cov else None
    status = torch.zeros(n_opt, dtype=torch.int32, device=dev)
    nbytes = int(lib().aoc_filter_gains_scratch_bytes(n_opt, T))
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    p = problem.c_problem(n_opt)
    check(lib().aoc_filter_gains(C.byref(p), n_opt, _ptr(nominal), _ptr(S0), C.byref(nz) if nz is not None else None, rho_c,
                                 mask, _ptr(filt), _ptr(cov), _ptr(status), _ptr(scratch), nbytes), "aoc_filter_gains")
    return filt, cov, status


def filter_gains_device(problem, xx_opt, uu_opt, Sigma0, sigma, rho, measured=None, to_host=True):
    """filter_gains for n_opt optima in ONE call, on the device (aoc_filter_gains), and for a filter that measures only some
    of the six channels: y = H dx + v, H the rows `measured` of the identity (a sequence of channel indices; None = all), V =
    diag(rho^2) of those channels — the rho of an unmeasured channel is not read.  The measurement update takes one scalar
    measurement at a time (include/aoc.h), so its values differ from filter_gains' Joseph form in the last digits.
    xx_opt (6,T) or (n_opt,6,T), uu_opt likewise; Sigma0 (6,6) or (n_opt,6,6), symmetric (checked here); sigma (6,) or None.
    Returns L (n_opt,6,6,T), P_prior (n_opt,6,6,T), P_post (n_opt,6,6,T), status (n_opt,) — numpy, or device tensors with
    to_host=False.  An unmeasured column of L is exactly +0.0."""
    torch = _torch()
    xo, uo = np.asarray(xx_opt, dtype=np.float64), np.asarray(uu_opt, dtype=np.float64)
    if xo.ndim == 2:
        xo, uo = xo[None], uo[None]
    n_opt, T = xo.shape[0], problem.T
    if xo.shape != (n_opt, 6, T) or uo.shape != (n_opt, 2, T):
        raise ValueError("xx_opt must be (6,T) or (n_opt,6,T) with T = %d, uu_opt likewise" % T)
    mask = _measured_mask(measured)
    nominal = torch.from_numpy(ensemble_nominal(xo, uo, np.zeros((n_opt, 2, 6, T)))).to(problem.device)
    filt, cov, status = _filter_gains_device(problem, nominal, n_opt, Sigma0, sigma, rho, mask, True)
    iu = torch.as_tensor(np.concatenate([_ENV_TRI[0] * 6 + _ENV_TRI[1], _ENV_TRI[1] * 6 + _ENV_TRI[0]]), device=problem.device)
    full = []
    for half in (cov[:, :, :21], cov[:, :, 21:]):
        P = torch.empty((n_opt, T, 36), dtype=torch.float64, device=problem.device)
        P[:, :, iu] = torch.cat([half, half], dim=2)
        full.append(P.reshape(n_opt, T, 6, 6).permute(0, 2, 3, 1).contiguous())
    out = (filt.reshape(n_opt, T, 6, 6).permute(0, 2, 3, 1).contiguous(), full[0], full[1], status)
    return tuple(t.cpu().numpy() for t in out) if to_host else out


def _ens_summary(torch, v):
    """mean / max / quantiles over the members (rows) of one optimum, reduced on the device"""
    q = torch.quantile(v, torch.tensor(ENS_QUANTILES, dtype=v.dtype, device=v.device), dim=0)
    out = dict(mean=v.mean(dim=0), max=v.max(dim=0).values)
    out.update({"q%02d" % round(100 * f): q[i] for i, f in enumerate(ENS_QUANTILES)})
    return {k: a.cpu().numpy() for k, a in out.items()}


def track_ensemble(problem, xx_opt, uu_opt, x0_reg=None, delta=None, KK=None, sigma=None, seed=20260405, first=0,
                   step0=0, members_per_opt=None, trajectories=False, f32=False, to_host=True, envelope=False,
                   quantiles=None, bins=None, predict=False, mean0=None, Sigma0=None, predict_k=6.0, rho=None, filter=None,
                   ehat0=None, measured=None, predict_joint=False, u_min=None, u_max=None, u_rate=None, est_input=None):
    """Closed-loop tracking ensemble about shared optima (aoc_track_ensemble): the loop of lqr_tracking.py:279-281 for B
    members, u_t = u_opt_t + K_t (x_t - x_opt_t), x_{t+1} = step(x_t, u_t) + d_t, reduced to per-member statistics on
    the device; the optimum and its gains are stored once per optimum, not once per member.
    problem: BatchProblem with the tracking weights (lqr_tracking.py:324-328): they weigh the gains (KK=None) and the
    cost statistic.  xx_opt (6,T) or (n_opt,6,T), uu_opt likewise.  Members: x0_reg (B,6), or delta (B,6) added to sample
    0 of each member's optimum (lqr_tracking.py:265); member b belongs to optimum b // members_per_opt (ensemble_groups).
    KK=None: gains from ONE aoc_lqr_tracking call on the n_opt optima; KK (n_opt,2,6,T) (or (2,6,T)): used as is.
    sigma (6,) or None: std of the disturbance d_t drawn on the device, a function of (seed, first + b, step0 + t) —
    mpc.noise_draws(seed, step0 + t, first, B, sigma) restates it.  trajectories: also return xx_reg (B,6,T) (f32:
    stored as float32 on the device; not with sigma), uu_reg (B,2,T), dist (B,6,T) — numpy, or device tensors with
    to_host=False.
    Returns dict(max_dx (B,6), max_du (B,2), cost (B,), final_dx (B,6), first_bad (B,) int, status (B,), stats (B,16),
    members_per_opt, group (B,), summary: per optimum dict(n, n_bad = members with first_bad < T, max_dx / final_dx /
    cost: mean, max, q50, q90, q99 over the members — final_dx signed —, reduced with torch on the device)).
    envelope=True (aoc_track_ensemble_envelope; every other output keeps its bits): also `envelope`, per optimum the
    reduction over its members at every sample, dict(n (T,) int = members still in the domain, min_dx / max_dx (6,T),
    min_du / max_du (2,T; sample T-1: +inf / -inf), mean_dx (6,T), cov_dx (6,6,T) (population covariance; NaN where
    n = 0), raw (T,44) = the device's record, see envelope_merge / envelope_moments).
    quantiles=(0.05, 0.5, 0.95) (aoc_track_ensemble_histogram; every other output keeps its bits): quantile tubes over the
    members at every sample, from a 64-bin histogram per (optimum, sample, channel dx[0..5], du[0..1]) counted on the
    device.  bins=None: two passes over the same members — the envelope call first (`envelope` is returned as above),
    histogram_bins of its min / max, then the histogram call, which bins exactly the values the first pass saw; bins
    (n_opt,T,8,2) (or (T,8,2)) = (lo, inv_w): the caller's own — fixed corridors, or the common bins of a sharded job,
    whose counts histogram_merge adds — and no envelope call (unless envelope=True asks for it).  Adds, each a list per
    optimum: hist (T,8,64) int32, bins (T,8,2), tube (len(quantiles),8,T) and tube_width (8,T) (histogram_quantiles:
    bin midpoints and the bin width, the resolution), and `quantiles` as given.
    predict=True (aoc_track_covariance; every other output keeps its bits): also `predicted`, per optimum what linear theory
    gives for the same loop, dict(mean_dx (6,T), cov_dx (6,6,T), mean_du (2,T), cov_du (2,2,T), raw (T,32)) as
    predict_covariance, and `predicted_status` (n_opt,).  mean0 (6,) / (n_opt,6) and Sigma0 (6,6) / (n_opt,6,6): the
    moments of dx at sample 0; None: the population mean and covariance of each group's own initial deviations, computed
    on the host.  The disturbance is the call's own sigma.
    bins="predicted" (with quantiles=): the bins are histogram_bins_predicted of that prediction, mean -+ predict_k std, so
    the histogram call is the ONLY pass over the members — no envelope call unless envelope=True asks for it — and
    `predicted` is returned as well.
    filter=L (6,6,T) or (n_opt,6,6,T) (aoc_track_ensemble_lqg; filter_gains computes such gains): no member feeds back its
    true state but a Kalman estimate from noisy measurements, y_t = dx_t + v_t, e^+_t = e^-_t + L_t (y_t - e^-_t),
    u_t = u_opt_t + K_t e^+_t, e^-_{t+1} = F_t e^+_t + c_t (include/aoc.h).  rho (6,) or None: std of the measurement noise
    v_t, drawn on the device — mpc.noise_draws(seed, step0 + t, first, B, rho, 1) restates it —; None: v = 0.  ehat0 (6,) or
    (n_opt,6): the prior estimate of dx_0 of each optimum's members, None = 0.  Every output above is then that of this
    loop; added: est_stats (B,12), max_e (B,6) = max_t |e_t| and sum_e2 (B,6) = sum_t e_t^2 of the estimation error e_t =
    dx_t - e^+_t, and with trajectories=True xhat (B,6,T) = x_opt_t + e^+_t and meas (B,6,T) = v_t.  rho= or ehat0= without
    filter=, and filter= together with envelope=, quantiles= or predict=, raise ValueError.
    filter="device" (aoc_filter_gains, then aoc_track_ensemble_lqg on the same stream): the gains of all n_opt optima are
    computed on the device by ONE call and handed over as they lie — nothing of L visits the host.  The filter is built on
    Sigma0 (6,6) / (n_opt,6,6), the covariance of the prior estimate's error (required: ValueError without it), the call's
    sigma and rho (required), and measures the channels `measured` (a sequence of indices; None = all; filter_gains_device).
    The members' measurement noise is still drawn in all six channels with rho.  Adds `filter_status` (n_opt,).
    predict_joint=True (with filter=; aoc_track_covariance_lqg on the same gains; every other output keeps its bits): also
    `predicted_joint`, per optimum what linear theory gives for THIS loop — lqg_covariance_moments' dict, the joint moments
    of dx and of the estimation error e — and `predicted_joint_status` (n_opt,).  mean0 / Sigma0 = None: the population
    moments of each group's own initial deviations, as for predict=True (with filter="device", Sigma0 is the filter's
    prior as well).  ValueError without filter=.
    u_min, u_max, u_rate (each (2,) = thrust, pitching moment; None or an infinite component: unbounded; u_rate in input
    units per second) (aoc_track_ensemble_limited): the demand v_t = u_opt_t + K_t dx_t is cut to [u_min, u_max] and, from
    sample 1 on, to within u_rate * dt of the input before (include/aoc.h) — and the cut input is what the plant and every
    output above see; envelope=, quantiles=, trajectories= and f32= work as before, on this loop.  With none of the three
    the calls and the result are what they were.  Adds sat (B,6) = per channel the number of cut samples, the first cut
    sample (T if none) and max_t |v - u|; sat_count, per optimum (T,2) int32 = the members cut at each sample among those
    still in the domain (sat_count_merge joins calls cut by `first=`); `limits` = dict(u_min, u_max, u_rate); and
    summary[k]["frac_cut"] (2,) = the share of members cut at least once.  predict=True and bins="predicted" stay allowed,
    but describe the UNLIMITED linear loop.
    filter= together with a limit and est_input="applied" | "demanded" (aoc_track_ensemble_lqg_limited): the demand
    v_t = u_opt_t + K_t e^+_t of the estimator's loop is cut in the same way, and est_input says what the estimator's
    prediction is told — "applied": the cut input, e^-_{t+1} = F_t e^+_t + c_t + B_t (u_t - v_t) where the sample is cut, which
    restores the separation of the linear loop; "demanded": the estimator of filter= as it is, F = A + B K, which a cut
    misleads.  Works with filter="device", rho=, ehat0=, trajectories= and f32=, not with envelope= or quantiles= (as for
    filter=).  The result holds the outputs of filter= and sat, sat_count, limits and summary[k]["frac_cut"] as above, and
    `est_input` as given.  predict_joint=True stays allowed but describes the loop WITHOUT limits.  filter= together with a
    limit and no est_input= raises ValueError (the choice is the caller's), so does est_input= without both a filter and a
    limit, or a name other than the two."""
    lqg = filter is not None
    limited = u_min is not None or u_max is not None or u_rate is not None
    if limited and lqg and est_input is None:
        raise ValueError("filter= (the estimator in the loop) does not combine with u_min= / u_max= / u_rate= unless est_input= "
                         "says what its prediction is told: \"applied\" (the cut input) or \"demanded\" (F = A + B K as it "
                         "is, which is wrong once the input is cut)")
    if est_input is not None:
        if not (limited and lqg):
            raise ValueError("est_input= goes with filter= and a limit (u_min= / u_max= / u_rate=)")
        if est_input not in ("applied", "demanded"):
            raise ValueError('est_input=%r: the names are "applied" and "demanded"' % (est_input,))
    if limited:
        lim_lo, lim_hi, lim_rate = actuator_limits(u_min, u_max, u_rate)
    if predict_joint and not lqg:
        raise ValueError("predict_joint=True goes with filter= (the prediction of the LQG loop); predict=True is the "
                         "prediction of the loop that feeds back the true state")
    device_gains = isinstance(filter, str)
    if device_gains:
        if filter != "device":
            raise ValueError('filter=%r: the only name is "device"' % (filter,))
        if Sigma0 is None or rho is None:
            raise ValueError('filter="device" needs Sigma0= (the covariance of the prior estimate\'s error) and rho=')
        mask = _measured_mask(measured)
    elif measured is not None:
        raise ValueError('measured= goes with filter="device"')
    if not lqg and (rho is not None or ehat0 is not None):
        raise ValueError("rho= and ehat0= go with filter= (the gains of the estimator, e.g. from filter_gains)")
    if lqg and (envelope or quantiles is not None or predict or bins is not None):
        raise ValueError("filter= (the estimator in the loop) does not combine with envelope=, quantiles= or predict=")
    torch = _torch()
    dev = problem.device
    xo, uo = np.asarray(xx_opt, dtype=np.float64), np.asarray(uu_opt, dtype=np.float64)
    if xo.ndim == 2:
        xo, uo = xo[None], uo[None]
    n_opt, T = xo.shape[0], problem.T
    if xo.shape != (n_opt, 6, T) or uo.shape != (n_opt, 2, T):
        raise ValueError("xx_opt must be (6,T) or (n_opt,6,T) with T = %d, uu_opt likewise" % T)
    if (x0_reg is None) == (delta is None):
        raise ValueError("give the members either as x0_reg (B,6) or as delta (B,6)")
    m = np.asarray(x0_reg if delta is None else delta, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != 6:
        raise ValueError("x0_reg / delta must be (B,6)")
    B = m.shape[0]
    mpo, group = ensemble_groups(B, n_opt, members_per_opt)
    x0 = m if delta is None else xo[group, :, 0] + m
    if KK is None:
        KK, _ = tracking_gains(problem, xo, uo)
    else:
        KK = np.asarray(KK, dtype=np.float64)
        KK = KK[None] if KK.ndim == 3 else KK
    nominal = torch.from_numpy(ensemble_nominal(xo, uo, KK)).to(dev)
    x0t = pack_vec(x0, dev)
    nt = ntiles(B)
    stats = torch.empty((nt, ENS_NSTAT, TILE), dtype=torch.float64, device=dev)
    status = torch.zeros(nt * TILE, dtype=torch.int32, device=dev)
    xr = ur = ds = None
    if trajectories:
        xr, ur = alloc_tiled(B, T, 6, dev, f32=f32), alloc_tiled(B, T, 2, dev)
        ds = alloc_tiled(B, T, 6, dev)
    nz = None
    if sigma is not None:
        nz = _lib.MpcNoise(int(seed), int(step0), int(first), (C.c_double * 6)(*np.asarray(sigma, dtype=np.float64).tolist()))
    p = problem.c_problem(B, x_out_f32=int(bool(f32)))
    nzp = C.byref(nz) if nz is not None else None
    if limited:
        lim = _lib.ActuatorLimits((C.c_double * 2)(*lim_lo.tolist()), (C.c_double * 2)(*lim_hi.tolist()),
                                  (C.c_double * 2)(*lim_rate.tolist()))
        sat = torch.empty((nt, SAT_NSTAT, TILE), dtype=torch.float64, device=dev)
        sat_count = torch.empty((n_opt, T, 2), dtype=torch.int32, device=dev)

        def limited_call(mode, out, st_, sts_, first_call, bins_d=None, env_d=None, hist_d=None):
            """One aoc_track_ensemble_limited call; sat and sat_count are those of the first call over the members"""
            sat_d = sat if first_call else torch.empty_like(sat)
            cnt_d = sat_count if first_call else None
            nbytes = int(lib().aoc_ensemble_limited_scratch_bytes(mode, B, T, mpo, int(first_call)))
            scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
            check(lib().aoc_track_ensemble_limited(C.byref(p), mode, n_opt, mpo, _ptr(nominal), _ptr(x0t), nzp, C.byref(lim),
                                                   _ptr(bins_d), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(st_),
                                                   _ptr(sts_), _ptr(sat_d), _ptr(cnt_d), _ptr(env_d), _ptr(hist_d),
                                                   _ptr(scratch) if nbytes else None, nbytes), "aoc_track_ensemble_limited")
    hist = quantiles is not None
    bins_predicted = isinstance(bins, str)
    if bins_predicted:
        if bins != "predicted" or not hist:
            raise ValueError('bins=%r: the only name is "predicted", and it goes with quantiles=' % (bins,))
        predict = True
    if predict:
        dx0 = x0 - xo[group, :, 0]
        if mean0 is None:
            mean0 = np.stack([dx0[group == k].mean(axis=0) for k in range(n_opt)])
        if Sigma0 is None:
            Sigma0 = np.stack([np.cov(dx0[group == k].T, bias=True).reshape(6, 6) for k in range(n_opt)])
            Sigma0 = 0.5 * (Sigma0 + Sigma0.transpose(0, 2, 1))
        pred_raw, pred_status = _predict_covariance(problem, nominal, n_opt, mean0, Sigma0, sigma)
        if bins_predicted:
            bins = histogram_bins_predicted(pred_raw, predict_k)
    if hist:
        quantiles = tuple(float(f) for f in np.atleast_1d(np.asarray(quantiles, dtype=np.float64)))
        if bins is not None:
            bins = np.asarray(bins, dtype=np.float64)
            bins = bins[None] if bins.ndim == 3 else bins
            if bins.shape != (n_opt, T, HIST_NCH, 2):
                raise ValueError("bins must be (n_opt,T,%d,2) = %s, got %s" % (HIST_NCH, (n_opt, T, HIST_NCH, 2), bins.shape))
        else:
            envelope = True
    elif bins is not None:
        raise ValueError("bins= goes with quantiles=")
    if envelope and limited:
        env = torch.empty((n_opt, T, ENV_NREC), dtype=torch.float64, device=dev)
        limited_call(_lib.ENS_MODE_ENVELOPE, (xr, ur, ds), stats, status, True, env_d=env)
    elif envelope:
        env = torch.empty((n_opt, T, ENV_NREC), dtype=torch.float64, device=dev)
        nbytes = int(lib().aoc_ensemble_envelope_scratch_bytes(B, T, mpo))
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
        check(lib().aoc_track_ensemble_envelope(C.byref(p), n_opt, mpo, _ptr(nominal), _ptr(x0t), nzp, _ptr(xr), _ptr(ur),
                                                _ptr(ds), _ptr(stats), _ptr(status), _ptr(env), _ptr(scratch), nbytes),
              "aoc_track_ensemble_envelope")
        # the 352 B per tile and sample go back before the histogram's 512 B are taken; the kernels run on the stream of
        # the caching allocator that frees them, so a later owner of the memory is ordered behind them
        del scratch
    if hist:
        # the second pass over the same members: with the envelope's call before it, it repeats the statistics only (same
        # bits, into buffers of its own); with the caller's bins it is the one call and writes everything
        if bins is None:
            bins = histogram_bins(env.cpu().numpy())
        bins_d = torch.from_numpy(np.ascontiguousarray(bins)).to(dev)
        hist_d = torch.empty((n_opt, T, HIST_NCH, HIST_NBIN), dtype=torch.int32, device=dev)
        first_call = not envelope
        h_stats, h_status = (stats, status) if first_call else (torch.empty_like(stats), torch.zeros_like(status))
        h_out = (xr, ur, ds) if first_call else (None, None, None)
        if limited:
            limited_call(_lib.ENS_MODE_HISTOGRAM, h_out, h_stats, h_status, first_call, bins_d=bins_d, hist_d=hist_d)
        else:
            nbytes = int(lib().aoc_ensemble_histogram_scratch_bytes(B, T, mpo))
            scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
            check(lib().aoc_track_ensemble_histogram(C.byref(p), n_opt, mpo, _ptr(nominal), _ptr(x0t), nzp, _ptr(bins_d),
                                                     _ptr(h_out[0]), _ptr(h_out[1]), _ptr(h_out[2]), _ptr(h_stats),
                                                     _ptr(h_status), _ptr(hist_d), _ptr(scratch) if nbytes else None, nbytes),
                  "aoc_track_ensemble_histogram")
            del scratch
    if lqg:
        if device_gains:
            filt_d, _, filt_status = _filter_gains_device(problem, nominal, n_opt, Sigma0, sigma, rho, mask, False)
        else:
            filt_d = _filter_to_device(filter, n_opt, T, dev)   # [opt][t][36]
        e0_d = None
        if ehat0 is not None:
            e0 = np.asarray(ehat0, dtype=np.float64)
            e0 = np.broadcast_to(e0, (n_opt, 6)) if e0.ndim == 1 else e0
            if e0.shape != (n_opt, 6):
                raise ValueError("ehat0 must be (6,) or (n_opt,6) with n_opt = %d, got %s" % (n_opt, e0.shape))
            e0_d = _dev_f64(np.ascontiguousarray(e0), dev)
        rho_c = None
        if rho is not None:
            rho_c = (C.c_double * 6)(*np.asarray(rho, dtype=np.float64).reshape(6).tolist())
            if nz is None:                                      # the seed lives in the disturbance model: one that adds nothing
                nz = _lib.MpcNoise(int(seed), int(step0), int(first), (C.c_double * 6)(*([0.0] * 6)))
                nzp = C.byref(nz)
        est_stats = torch.empty((nt, LQG_NSTAT, TILE), dtype=torch.float64, device=dev)
        xh = ms = None
        if trajectories:
            xh, ms = alloc_tiled(B, T, 6, dev), alloc_tiled(B, T, 6, dev)
        if limited:
            nbytes = int(lib().aoc_track_ensemble_lqg_limited_scratch_bytes(B, n_opt, T, mpo, 1))
            scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
            told = _lib.EST_INPUT_APPLIED if est_input == "applied" else _lib.EST_INPUT_DEMANDED
            check(lib().aoc_track_ensemble_lqg_limited(C.byref(p), n_opt, mpo, _ptr(nominal), _ptr(filt_d), _ptr(x0t), _ptr(e0_d),
                                                       nzp, rho_c, C.byref(lim), told, _ptr(xr), _ptr(ur), _ptr(xh), _ptr(ds),
                                                       _ptr(ms), _ptr(stats), _ptr(est_stats), _ptr(sat), _ptr(sat_count),
                                                       _ptr(status), _ptr(scratch), nbytes), "aoc_track_ensemble_lqg_limited")
        else:
            nbytes = int(lib().aoc_track_ensemble_lqg_scratch_bytes(n_opt, T))
            scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
            check(lib().aoc_track_ensemble_lqg(C.byref(p), n_opt, mpo, _ptr(nominal), _ptr(filt_d), _ptr(x0t), _ptr(e0_d), nzp,
                                               rho_c, _ptr(xr), _ptr(ur), _ptr(xh), _ptr(ds), _ptr(ms), _ptr(stats),
                                               _ptr(est_stats), _ptr(status), _ptr(scratch), nbytes), "aoc_track_ensemble_lqg")
        del scratch
        if predict_joint:
            dx0 = x0 - xo[group, :, 0]
            jm0 = mean0 if mean0 is not None else np.stack([dx0[group == k].mean(axis=0) for k in range(n_opt)])
            jS0 = Sigma0
            if jS0 is None:
                jS0 = np.stack([np.cov(dx0[group == k].T, bias=True).reshape(6, 6) for k in range(n_opt)])
                jS0 = 0.5 * (jS0 + jS0.transpose(0, 2, 1))
            joint_raw, joint_status = _predict_covariance_lqg(problem, nominal, filt_d, n_opt, jm0, ehat0, jS0, sigma, rho)
    elif not envelope and not hist and limited:
        limited_call(_lib.ENS_MODE_STATS, (xr, ur, ds), stats, status, True)
    elif not envelope and not hist:
        check(lib().aoc_track_ensemble(C.byref(p), n_opt, mpo, _ptr(nominal), _ptr(x0t), nzp,
                                       _ptr(xr), _ptr(ur), _ptr(ds), _ptr(stats), _ptr(status)), "aoc_track_ensemble")
    sv = unpack_vec(stats, B)                                   # (B,16) on the device
    first_bad = sv[:, 15].to(torch.int64)
    summary = []
    for g in range(n_opt):
        sl = slice(g * mpo, min((g + 1) * mpo, B))
        summary.append(dict(n=sl.stop - sl.start, n_bad=int((first_bad[sl] < T).sum()),
                            max_dx=_ens_summary(torch, sv[sl, 0:6]), final_dx=_ens_summary(torch, sv[sl, 9:15]),
                            cost=_ens_summary(torch, sv[sl, 8])))
    s = sv.cpu().numpy()
    out = dict(max_dx=s[:, 0:6], max_du=s[:, 6:8], cost=s[:, 8], final_dx=s[:, 9:15], first_bad=s[:, 15].astype(np.int64),
               status=status[:B].cpu().numpy(), stats=s, members_per_opt=mpo, group=group, summary=summary)
    if limited:
        sa = unpack_vec(sat, B).cpu().numpy()
        for g, sm in enumerate(summary):
            sm["frac_cut"] = frac_cut(sa[g * mpo:min((g + 1) * mpo, B)])
        out.update(sat=sa, sat_count=list(sat_count.cpu().numpy()),
                   limits=dict(u_min=lim_lo, u_max=lim_hi, u_rate=lim_rate))
        if lqg:
            out["est_input"] = est_input
    if lqg:
        es = unpack_vec(est_stats, B).cpu().numpy()
        out.update(est_stats=es, max_e=es[:, 0:6], sum_e2=es[:, 6:12])
        if device_gains:
            out["filter_status"] = filt_status.cpu().numpy()
        if predict_joint:
            out.update(predicted_joint=[lqg_covariance_moments(r) for r in joint_raw], predicted_joint_status=joint_status)
    if envelope:
        out["envelope"] = [_envelope_dict(r) for r in env.cpu().numpy()]
    if predict:
        out.update(predicted=[_covariance_dict(r) for r in pred_raw], predicted_status=pred_status)
    if hist:
        counts = hist_d.cpu().numpy()
        tube, width = histogram_quantiles(counts, bins, quantiles)
        out.update(quantiles=quantiles, hist=list(counts), bins=list(bins), tube=list(tube.transpose(1, 0, 2, 3)),
                   tube_width=list(width))
    if trajectories:
        xd = unpack(xr, B)
        xd[:, :, 0] = _dev_f64(x0, dev)                         # sample 0 is the fp64 x0, as everywhere
        host = (lambda t: t.cpu().numpy()) if to_host else (lambda t: t)
        out.update(xx_reg=host(xd), uu_reg=host(unpack(ur, B)), dist=host(unpack(ds, B)))
        if lqg:
            out.update(xhat=host(unpack(xh, B)), meas=host(unpack(ms, B)))
    return out


def ltv_lqr_batch(AA, BB, QQ, RR, SS, QQf, x0, qq=None, rr=None, qqf=None, device="cuda:0"):
    """Generic ltv_LQR for nb problems (reference optcon.py:533-771).  Time-major inputs per problem:
    AA (nb,T,6,6), BB (nb,T,6,2), QQ (nb,T,6,6), RR (nb,T,2,2), SS (nb,T,2,6), QQf (nb,6,6), x0 (nb,6),
    affine terms qq (nb,T,6), rr (nb,T,2), qqf (nb,6) or None.  Returns KK (nb,T,2,n), PP (nb,T,n,n),
    xx (nb,T,6), uu (nb,T,2), nreg (nb,), nsing (nb,)."""
    torch = _torch()
    aug = qq is not None or rr is not None or qqf is not None  # optcon.py:614
    n = 7 if aug else 6
    d = lambda a: None if a is None else _dev_f64(a, device)
    A, Bm, Q, R, S, Qf, X0 = (d(a) for a in (AA, BB, QQ, RR, SS, QQf, x0))
    nb, T = A.shape[0], A.shape[1]
    q, r, qf = d(qq), d(rr), d(qqf)
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device=A.device)
    KK, PP, xx, uu = mk(nb, T, 2, n), mk(nb, T, n, n), mk(nb, T, 6), mk(nb, T, 2)
    nreg = torch.zeros(nb, dtype=torch.int32, device=A.device)
    nsing = torch.zeros(nb, dtype=torch.int32, device=A.device)
    st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
    check(lib().aoc_ltv_lqr(nb, T, int(aug), _ptr(A), _ptr(Bm), _ptr(Q), _ptr(R), _ptr(S), _ptr(Qf), _ptr(X0), _ptr(q),
                            _ptr(r), _ptr(qf), _ptr(KK), _ptr(PP), _ptr(xx), _ptr(uu), _ptr(nreg), _ptr(nsing), st),
          "aoc_ltv_lqr")
    return tuple(t.cpu().numpy() for t in (KK, PP, xx, uu, nreg, nsing))



class NewtonBatchSolverF32:
    """The batched Newton iteration in float32 arithmetic (BASELINE configs[2]): every array float32,
    every operation float32 (`aoc_*_f32`).  Not the parity path — the reference computes in fp64 —
    but the same algorithm; used to measure how much accuracy float32 costs (tests/test_gpu_f32.py).
    Interface: the subset of NewtonBatchSolver needed for fixed-iteration runs."""

    def __init__(self, problem, B, params=None):
        torch = _torch()
        self.problem, self.B, self.T = problem, int(B), problem.T
        self.params = params if params is not None else make_params()
        dev = problem.device
        self.nt = ntiles(self.B)
        self.Bp = self.nt * TILE
        f32 = torch.float32
        self.ref32 = problem.ref.to(f32).contiguous()
        self.xb = [alloc_tiled(B, self.T, 6, dev, zero=True, f32=True) for _ in range(2)]
        self.ub = [alloc_tiled(B, self.T, 2, dev, zero=True, f32=True) for _ in range(2)]
        self.ws = torch.empty((lib().aoc_workspace_bytes_f32(self.B, self.T) + 3) // 4, dtype=f32, device=dev)
        f = lambda: torch.zeros(self.Bp, dtype=f32, device=dev)
        self.J = [f(), f()]
        self.descent, self.stepsize = f(), f()
        self.ntrials = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        self.x0 = torch.zeros((self.nt, 6, TILE), dtype=f32, device=dev)
        self.cur = self.jcur = self.kk = 0

    def _p(self):
        p = self.problem.c_problem(self.B, x_in_f32=1, x_out_f32=1)
        p.ref = self.ref32.data_ptr()
        return p

    def set_initial_rollout(self, x0, uu):
        """x0 (B,6), uu (B,2,T): the initial iterate is the open-loop rollout of uu from x0 (config 3:
        warm start from a saved optimum)."""
        torch = _torch()
        dev = self.problem.device
        self.x0.copy_(pack_vec(x0, dev).to(torch.float32))
        ut = pack(uu, dev, f32=True)
        p = self._p()
        check(lib().aoc_rollout_cost_f32(C.byref(p), _ptr(self.x0), _ptr(ut), None, None, _ptr(self.xb[0]),
                                         _ptr(self.ub[0]), _ptr(self.J[0]), _ptr(self.status)), "aoc_rollout_cost_f32")
        self.cur = self.jcur = self.kk = 0

    def set_initial_from_x0(self, x0, kp=5.0, kt=2.5):
        torch = _torch()
        dev = self.problem.device
        self.x0.copy_(pack_vec(x0, dev).to(torch.float32))
        p = self._p()
        check(lib().aoc_initial_trajectory_f32(C.byref(p), float(kp), float(kt), _ptr(self.x0), _ptr(self.xb[0]),
                                               _ptr(self.ub[0])), "aoc_initial_trajectory_f32")
        check(lib().aoc_traj_cost_f32(C.byref(p), _ptr(self.xb[0]), _ptr(self.ub[0]), _ptr(self.x0), _ptr(self.J[0])),
              "aoc_traj_cost_f32")
        self.cur = self.jcur = self.kk = 0

    def iterate(self, kk=None):
        if kk is None:
            kk = self.kk
        p = self._p()
        c, n = self.cur, 1 - self.cur
        jc, jn = self.jcur, 1 - self.jcur
        check(lib().aoc_newton_iterate_f32(C.byref(p), C.byref(self.params), int(kk), _ptr(self.xb[c]), _ptr(self.ub[c]),
                                           _ptr(self.x0), _ptr(self.J[jc]), _ptr(self.ws), self.ws.numel() * 4, _ptr(self.xb[n]),
                                           _ptr(self.ub[n]), _ptr(self.J[jn]), _ptr(self.descent), _ptr(self.stepsize),
                                           _ptr(self.ntrials), _ptr(self.status)), "aoc_newton_iterate_f32")
        self.cur, self.jcur, self.kk = n, jn, kk + 1

    def join(self):
        """(interface shared with TwoStreamNewtonSolver: one stream, nothing to wait for)"""

    def current(self):
        xx = unpack(self.xb[self.cur], self.B)
        xx[:, :, 0] = unpack_vec(self.x0, self.B).to(xx.dtype)
        return xx.cpu().numpy(), unpack(self.ub[self.cur], self.B).cpu().numpy()

    def scalars(self):
        B = self.B
        g = lambda t: t[:B].double().cpu().numpy()
        return dict(cost=g(self.J[1 - self.jcur]), descent=g(self.descent), stepsize=g(self.stepsize),
                    ntrials=self.ntrials[:B].cpu().numpy(), cost_new=g(self.J[self.jcur]),
                    status=self.status[:B].cpu().numpy())
