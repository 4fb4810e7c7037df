"""Host-side mirror of the reference's ``Hqp_IpMatrix`` plugin interface
(hqp/Hqp_IpMatrix.h:42-89) over the C ABI of include/hqpkkt.h.

Same method names, argument meaning and error behaviour as the reference:

    m = IpSpBKP()            # Hqp_IpSpBKP    (hqp/Hqp_IpSpBKP.C)
    m = IpRedSpBKP()         # Hqp_IpRedSpBKP (hqp/Hqp_IpRedSpBKP.C)
    m.init(qp)               # structure: RCM, mat_sbw, symbolic factorisation
    m.update(qp)             # new values, same pattern
    m.factor(qp, z, w)
    res = m.solve(qp, z, w, r1, r2, r3, r4, dx, dy, dz, dw)   # fills dx..dw
    m.step(...), m.residuum(...)

``qp`` is an :class:`hqp_amd.problems.Program` (the Hqp_Program data contract).
Vectors are numpy float64 arrays (host pointers, like Meschach ``VEC::ve``) or
torch CUDA tensors (device pointers, used in place) -- one kind per object,
chosen at construction (``device_vectors=True``).  A numerically singular system
raises :class:`SingularError`, the counterpart of ``m_error(E_SING, ...)``
(meschach/err.h:63,88) which the interior-point solvers catch
(hqp/Hqp_IpsMehrotra.C:525-536).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class KktError(RuntimeError):
    def __init__(self, code, where):
        super().__init__(f"hqpkkt status {code} in {where}: {_lib.strerror(code)}")
        self.code = code


class SingularError(KktError):
    """E_SING of the reference (meschach/err.h:88)."""


def _check(code, where):
    if code == _lib.OK:
        return
    if code == _lib.E_SING:
        raise SingularError(code, where)
    raise KktError(code, where)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a


class Hqp_IpMatrix:
    """Abstract base (hqp/Hqp_IpMatrix.h:42-89)."""

    _mode = None
    _name = None

    def __init__(self, device=0, device_vectors=False, mat_tol=1.0, mat_eps=1e-10,
                 pivot_eps=None, leaf_size=0, max_pivots=0, zd_policy=None, shard=None, slack_policy=None, small_fronts=True, upd_pingpong_mb=0,
                 amalgamation=False, ordering=0):
        L = _lib.lib()
        o = _lib.Opts()
        L.hqpkkt_default_opts(C.byref(o))
        o.mode = self._mode
        o.device = device
        o.loc = _lib.LOC_DEVICE if device_vectors else _lib.LOC_HOST
        o.tol, o.eps = mat_tol, mat_eps
        if pivot_eps is not None:
            o.pivot_eps = pivot_eps
        o.leaf_size, o.max_pivots = leaf_size, max_pivots
        if zd_policy is not None:
            o.zd_policy = zd_policy
        if slack_policy is not None:
            o.slack_policy = slack_policy
        o.no_small_fronts = 0 if small_fronts else 1
        o.upd_pingpong_mb = upd_pingpong_mb
        o.amalgamation = 1 if amalgamation else 0
        o.ordering = int(ordering)
        self._L = L
        self._h = C.c_void_p()
        self._device_vectors = bool(device_vectors)
        self._dev = int(device)
        _check(L.hqpkkt_create(C.byref(o), C.byref(self._h)), "create")
        self._keep = None
        self._xchg = None
        self.n = self.me = self.m = 0
        if shard is not None:
            if hasattr(shard, "fn"):  # hqp_amd.dist.RcclShard: stream-ordered RCCL collectives
                _check(L.hqpkkt_set_shard_stream(self._h, shard.rank, shard.world, shard.fn, shard._ctx), "set_shard_stream")
                self._xchg = shard
            else:
                self.set_shard(*shard)

    def set_shard(self, rank, count, exchange=None):
        """One system over ``count`` ranks (call before init()).  ``exchange(op,
        device_pointer, slot_elems, nslots)`` performs the collectives, see
        hqp_amd.dist.make_exchange and hqpkkt_set_shard in include/hqpkkt.h."""
        import sys
        import traceback

        def tramp(_ctx, op, buf, slot, nslots):
            try:
                exchange(op, buf, slot, nslots)
                return 0
            except Exception:  # never unwind through the C frames
                traceback.print_exc(file=sys.stderr)
                return 1

        cb = _lib.EXCHANGE_FN(tramp) if exchange is not None else C.cast(None, _lib.EXCHANGE_FN)
        _check(self._L.hqpkkt_set_shard(self._h, rank, count, cb, None), "set_shard")
        self._xchg = cb  # keep the thunk alive as long as the handle

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.hqpkkt_destroy(h)
            self._h = None

    # -- Tcl-visible members of the reference -------------------------------
    @property
    def mat_sbw(self):
        v = C.c_int()
        _check(self._L.hqpkkt_get_sbw(self._h, C.byref(v)), "get_sbw")
        return v.value

    def set_mat_tol(self, tol):
        _check(self._L.hqpkkt_set_tol(self._h, tol), "set_tol")

    def set_mat_eps(self, eps):
        _check(self._L.hqpkkt_set_eps(self._h, eps), "set_eps")

    def name(self):
        return self._name

    # -- pointer plumbing ------------------------------------------------------
    def _ptr(self, a, size, what, out=False):
        if a is None:
            if size:
                raise KktError(_lib.E_NULL, what)
            return None
        if self._device_vectors:
            if not (hasattr(a, "data_ptr") and a.is_cuda):
                raise TypeError(f"{what}: device_vectors=True needs torch CUDA float64 tensors")
            if a.numel() != size or str(a.dtype) != "torch.float64" or not a.is_contiguous():
                raise KktError(_lib.E_SIZES, what)
            return C.c_void_p(a.data_ptr())
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
            if out:
                raise TypeError(f"{what}: output must be a C-contiguous float64 numpy array")
            a = np.ascontiguousarray(a, dtype=np.float64)
            self._tmp.append(a)
        if a.size != size:
            raise KktError(_lib.E_SIZES, what)  # the reference asserts (Hqp_IpSpBKP.C:189-192)
        return C.c_void_p(a.ctypes.data)

    def _vecs(self, z, w, r1, r2, r3, r4, dx, dy, dz, dw, out=True):
        self._tmp = []
        n, me, m = self.n, self.me, self.m
        sizes = (m, m, n, me, m, m)
        ins = [self._ptr(a, s, nm) for a, s, nm in zip((z, w, r1, r2, r3, r4), sizes,
                                                      ("z", "w", "r1", "r2", "r3", "r4"))]
        outs = [self._ptr(a, s, nm, out=out) for a, s, nm in zip((dx, dy, dz, dw), (n, me, m, m),
                                                                 ("dx", "dy", "dz", "dw"))]
        return ins + outs

    # -- the plugin interface ----------------------------------------------------
    def _vec_in(self, a, size, what):
        """(pointer, what keeps it alive) of a caller's input vector of the entries on Q (the sparse Q, the dense stage
        Hessians): numpy, or a torch CUDA tensor with device_vectors=True; None is the null pointer."""
        if a is None:
            return C.c_void_p(None), None
        if self._device_vectors:
            if not (hasattr(a, "data_ptr") and a.is_cuda):
                raise TypeError(f"{what}: device_vectors=True needs torch CUDA float64 tensors")
            if a.numel() != size or str(a.dtype) != "torch.float64" or not a.is_contiguous():
                raise KktError(_lib.E_SIZES, what)
            return C.c_void_p(a.data_ptr()), a
        if hasattr(a, "data_ptr"):
            raise TypeError(f"{what}: torch tensors need device_vectors=True")
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != size:
            raise KktError(_lib.E_SIZES, what)
        return C.c_void_p(a.ctypes.data), a

    def _vec_out(self, size):
        """(pointer, vector) of a result of those entries: a numpy array, or a torch CUDA tensor with device_vectors=True."""
        if self._device_vectors:
            import torch
            v = torch.zeros(size, dtype=torch.float64, device=torch.device("cuda", self._dev))
            return C.c_void_p(v.data_ptr()), v
        v = np.zeros(size)
        return C.c_void_p(v.ctypes.data), v

    def _stream_sync(self, after=False):
        """Device vectors are read and written in the handle's stream: what torch has queued for them is over before the
        call, and (``after``) the handle's work before torch reads a result."""
        if self._device_vectors:
            import torch
            if after:
                torch.cuda.synchronize(self._dev)
            else:
                torch.cuda.current_stream(self._dev).synchronize()

    def init(self, qp):
        """Hqp_IpSpBKP::init (hqp/Hqp_IpSpBKP.C:76-114): analyse, then update."""
        self.analyze(qp)
        self.update(qp)

    def analyze(self, qp):
        """The symbolic phase alone (hqpkkt_analyze): host work, no device."""
        self.n, self.me, self.m = qp.dims
        arrs = []
        for (p, i, _x) in (qp.Q, qp.A, qp.C):
            arrs += [_i32(p), _i32(i)]
        self._keep = arrs
        sbw = C.c_int()
        ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
        _check(self._L.hqpkkt_analyze(self._h, self.n, self.me, self.m, *ptrs, C.byref(sbw)), "init")

    def update(self, qp):
        """Hqp_IpSpBKP::update (hqp/Hqp_IpSpBKP.C:117-136)."""
        vals = []
        for (_p, _i, x) in (qp.Q, qp.A, qp.C):
            if self._device_vectors and hasattr(x, "data_ptr"):
                vals.append(C.c_void_p(x.data_ptr()))
            elif self._device_vectors:
                import torch
                t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()
                self._keepvals = getattr(self, "_keepvals", []) + [t]
                vals.append(C.c_void_p(t.data_ptr()))
            else:
                a = np.ascontiguousarray(x, dtype=np.float64)
                self._keep.append(a)
                vals.append(C.c_void_p(a.ctypes.data) if a.size else None)
        _check(self._L.hqpkkt_set_values(self._h, *vals), "update")
        self._keepvals = []

    def factor(self, qp, z, w):
        self._tmp = []
        m = self.m
        _check(self._L.hqpkkt_factor(self._h, self._ptr(z, m, "z"), self._ptr(w, m, "w")), "factor")

    def step(self, qp, z, w, r1, r2, r3, r4, dx, dy, dz, dw):
        _check(self._L.hqpkkt_step(self._h, *self._vecs(z, w, r1, r2, r3, r4, dx, dy, dz, dw)), "step")

    def solve(self, qp, z, w, r1, r2, r3, r4, dx, dy, dz, dw):
        """Hqp_IpMatrix::solve (hqp/Hqp_IpMatrix.C:65-128); returns the residual."""
        res = C.c_double()
        _check(self._L.hqpkkt_solve(self._h, *self._vecs(z, w, r1, r2, r3, r4, dx, dy, dz, dw),
                                    C.byref(res)), "solve")
        return res.value

    def residuum(self, qp, z, w, r1, r2, r3, r4, dx, dy, dz, dw):
        """Hqp_IpMatrix::residuum (hqp/Hqp_IpMatrix.C:131-178)."""
        res = C.c_double()
        _check(self._L.hqpkkt_residual(self._h, *self._vecs(z, w, r1, r2, r3, r4, dx, dy, dz, dw, out=False),
                                       C.byref(res)), "residuum")
        return res.value

    # -- introspection ---------------------------------------------------------------
    def stats(self):
        s = _lib.Stats()
        _check(self._L.hqpkkt_get_stats(self._h, C.byref(s)), "get_stats")
        return s.asdict()

    def perm(self):
        """_QP2J of the reference: band position of each QP index."""
        p = np.zeros(self.stats()["dim"], dtype=np.int32)
        _check(self._L.hqpkkt_get_perm(self._h, C.c_void_p(p.ctypes.data)), "get_perm")
        return p

    def set_profile(self, on=True):
        _check(self._L.hqpkkt_set_profile(self._h, 1 if on else 0), "set_profile")

    def profile(self):
        """{kernel class: (summed device ms, launches)} since set_profile()."""
        ms = (C.c_double * 64)()
        ln = (C.c_longlong * 64)()
        k = min(self._L.hqpkkt_get_profile(self._h, 64, ms, ln), 64)
        return {self._L.hqpkkt_profile_class_name(c).decode(): (ms[c], ln[c]) for c in range(k)}

    def set_stream(self, hip_stream):
        _check(self._L.hqpkkt_set_stream(self._h, C.c_void_p(hip_stream)), "set_stream")

    def debug(self, what):
        k = C.c_longlong()
        _check(self._L.hqpkkt_debug_get(self._h, what, None, C.byref(k)), "debug_get")
        out = np.zeros(max(k.value, 1), dtype=np.int32)
        _check(self._L.hqpkkt_debug_get(self._h, what, C.c_void_p(out.ctypes.data), C.byref(k)), "debug_get")
        return out[: k.value]

    def franke(self, qp, eps=1e-10, max_iters=200, hot_start=0, qp_mu0=0.0):
        """Device-resident run of the reference's other interior-point solver, Hqp_IpsFranke
        (``hqpkkt_franke``): returns (x, y, z, w, info).  ``hot_start`` 1: Hqp_IpsFranke::hot_start
        from the iterate this handle's previous franke() call ended with.  ``qp_mu0``: the reference's
        interface variable of that name (cold start, hqp/Hqp_IpsFranke.C:167-173)."""
        return self.mehrotra(qp, eps, max_iters, hot_start, _entry="hqpkkt_franke", qp_mu0=qp_mu0)

    def mehrotra(self, qp, eps=1e-10, max_iters=200, hot_start=0, init_method=0, _entry="hqpkkt_mehrotra", qp_mu0=0.0):
        """Device-resident Mehrotra predictor-corrector solve of the QP, the restatement of
        hqp/Hqp_IpsMehrotra.C behind ``hqpkkt_mehrotra``: returns (x, y, z, w, info).
        init()/update() must have been called with ``qp``.  ``hot_start``: 0 cold start,
        1 Hqp_IpsMehrotra::hot_start from this handle's previous solve (which must have run
        with hot_start != 0), 2 cold start that keeps what the next hot start needs."""
        o = _lib.IpOpts()
        self._L.hqpkkt_default_ip_opts(C.byref(o))
        o.eps, o.max_iters, o.hot_start, o.init_method = eps, max_iters, int(hot_start), int(init_method)
        o.qp_mu0 = float(qp_mu0)

        def rowsum(csr, rows):  # sp_norm_inf (meschach/addon2_hqp.c:723-743)
            p, _i, x = csr
            if rows == 0 or len(x) == 0:
                return 0.0
            return float(np.add.reduceat(np.abs(np.r_[np.asarray(x, dtype=float), 0.0]),
                                         np.asarray(p[:-1], dtype=np.int64))[np.diff(p) > 0].max(initial=0.0))

        def ninf(v):
            if hasattr(v, "data_ptr"):  # torch tensor (device-resident problem data)
                return float(v.abs().max()) if v.numel() else 0.0
            return float(np.abs(v).max()) if len(v) else 0.0

        o.norm_Q, o.norm_C, o.norm_d = rowsum(qp.Q, qp.n), rowsum(qp.C, qp.m), ninf(qp.d)
        if getattr(qp, "norm_A", None) is not None:  # (the caller has released the blocks)
            norm_A = float(qp.norm_A)
        elif hasattr(qp, "F"):  # problems.DenseDocp: the dynamics rows are [fx fu | -1], the others are in E
            norm_A = max([float(abs(blk).sum(1).max()) + 1.0 for blk in qp.F] + [rowsum(qp.E, qp.me_rest)])
        else:
            norm_A = rowsum(qp.A, qp.me)
        o.norm_data = max(o.norm_Q, norm_A, o.norm_C, ninf(qp.c), ninf(qp.b), o.norm_d)
        res = _lib.IpResult()
        self._tmp = []
        if self._device_vectors:
            import torch
            dev = torch.device("cuda", self._dev)
            mk = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)
            cin = [v.to(dev) if hasattr(v, "data_ptr") else torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
                   for v in (qp.c, qp.b, qp.d)]
        else:
            mk = lambda k: np.zeros(k)
            cin = [np.ascontiguousarray(v, dtype=np.float64) for v in (qp.c, qp.b, qp.d)]
        x, y, z, w = mk(qp.n), mk(qp.me), mk(qp.m), mk(qp.m)
        ptrs = [self._ptr(a, k, nm) for a, k, nm in zip(cin + [x, y, z, w], (qp.n, qp.me, qp.m, qp.n, qp.me, qp.m, qp.m),
                                                      ("c", "b", "d", "x", "y", "z", "w"))]
        _check(getattr(self._L, _entry)(self._h, C.byref(o), *ptrs, C.byref(res)), _entry)
        return x, y, z, w, res.asdict()

    # -- the sparse Q where it lies on the device (hqpkkt_q_*, hqpkkt_lagrangian_gradient) ----------
    def _q_nnz(self):
        return int(self._keep[0][-1]) if self._keep and len(self._keep[0]) else 0

    def q_values(self):
        """Qx as it lies in the handle (hqpkkt_q_values): nnz(Q) values in the order of the analysed pattern."""
        p, v = self._vec_out(self._q_nnz())
        self._stream_sync()
        _check(self._L.hqpkkt_q_values(self._h, p), "q_values")
        return v

    def q_product(self, x):
        """y = Q x, Q symmetric from its stored upper entries (hqpkkt_q_product)."""
        px, kx = self._vec_in(x, self.n, "x")
        py, y = self._vec_out(self.n)
        self._stream_sync()
        _check(self._L.hqpkkt_q_product(self._h, px, py), "q_product")
        self._stream_sync(after=True)
        return y

    def q_row_stats(self, want_diag=True, want_offsum=True):
        """(diag, offsum) of Q (hqpkkt_q_row_stats): the stored q_ii (0.0 without one) and the sum of |q_ij| over j != i of
        the symmetric image; None for the one not wanted."""
        out = [self._vec_out(self.n) if w else (None, None) for w in (want_diag, want_offsum)]
        self._stream_sync()
        _check(self._L.hqpkkt_q_row_stats(self._h, out[0][0], out[1][0]), "q_row_stats")
        self._stream_sync(after=True)
        return out[0][1], out[1][1]

    def q_set_diagonal(self, d):
        """Q <- diag(d) on the stored pattern (hqpkkt_q_set_diagonal): Hqp_HL::init, sp_ident, a restart."""
        pd, kd = self._vec_in(d, self.n, "d")
        self._stream_sync()
        _check(self._L.hqpkkt_q_set_diagonal(self._h, pd), "q_set_diagonal")
        self._keep_qv = [kd]

    def q_gerschgorin(self, eps):
        """Hqp_HL_Gerschgorin::update on the sparse Q (hqpkkt_q_gerschgorin): q_ii <- max(q_ii, sum_{j != i} |q_ij| + eps)."""
        _check(self._L.hqpkkt_q_gerschgorin(self._h, float(eps)), "q_gerschgorin")

    def q_dscale_setup(self, eps):
        """Hqp_HL_DScale::setup (hqpkkt_q_dscale_setup): off-diagonals <- 0, q_ii <- max(q_ii, eps)."""
        _check(self._L.hqpkkt_q_dscale_setup(self._h, float(eps)), "q_dscale_setup")

    def q_dscale_update(self, s, y, gamma=0.2, bsize=0, want_v=False):
        """Hqp_HL_DScale::update on the diagonal of the sparse Q (hqpkkt_q_dscale_update) for the step ``s`` and the change
        ``y`` of the Lagrangian's gradient, in blocks of ``bsize`` variables (0: one block).  ``want_v``: returns v as
        applied, else None.  q_dscale_report() tells what every block did."""
        ps, ks = self._vec_in(s, self.n, "s")
        py, ky = self._vec_in(y, self.n, "y")
        u = _lib.DScaleUpdate()
        u.s, u.y, u.gamma, u.bsize = ps.value, py.value, float(gamma), int(bsize)
        v = None
        if want_v:
            pv, v = self._vec_out(self.n)
            u.v = pv.value
        self._stream_sync()
        _check(self._L.hqpkkt_q_dscale_update(self._h, C.byref(u)), "q_dscale_update")
        self._keep_qv = [ks, ky, v]
        if want_v:
            self._stream_sync(after=True)
        return v

    def q_dscale_report(self):
        """Per block of the last q_dscale_update() (hqpkkt_q_dscale_report), an array of shape (blocks, 8): sy, sqs, gamma,
        theta (1 where not damped), sv as used, first index, length and the outcome - 0 updated, 1 updated with damping,
        2 left alone (sv or sqs is zero), 3 left alone (sv or sqs is not finite).  Waits for the handle's stream."""
        k = C.c_longlong()
        out = np.zeros((1, _lib.HQPKKT_DSCALE_REPORT))
        e = self._L.hqpkkt_q_dscale_report(self._h, C.c_void_p(out.ctypes.data), 1, C.byref(k))
        if e == _lib.E_RANGE:
            out = np.zeros((k.value, _lib.HQPKKT_DSCALE_REPORT))
            e = self._L.hqpkkt_q_dscale_report(self._h, C.c_void_p(out.ctypes.data), k.value, C.byref(k))
        _check(e, "q_dscale_report")
        return out[: k.value]

    def q_blocks(self, bsize=-1):
        """(first, full) of hqpkkt_q_blocks: Hqp_HL_BFGS::next_block on the analysed pattern of Q.  ``first``: the blocks'
        first indices and n behind the last (blocks + 1 ints; empty for n = 0); ``full``: per block 1 where its whole upper
        triangle is stored.  ``bsize`` < 0 detects the blocks, 0 is one block, > 0 blocks of bsize.  Needs analyze() alone."""
        k = C.c_longlong()
        _check(self._L.hqpkkt_q_blocks(self._h, int(bsize), None, None, 0, C.byref(k)), "q_blocks")
        first, full = np.zeros(k.value + 1, dtype=np.int32), np.zeros(k.value, dtype=np.int32)
        if k.value:
            _check(self._L.hqpkkt_q_blocks(self._h, int(bsize), C.c_void_p(first.ctypes.data), C.c_void_p(full.ctypes.data), k.value, C.byref(k)), "q_blocks")
        return first[: k.value + 1 if k.value else 0], full

    def q_bfgs_update(self, s, y, gamma=0.1, alpha=1.0, bsize=-1, pattern=False, want_v=False, want_Qs=False, eigen_control=None):
        """Hqp_HL_BFGS::update on the sparse Q where it lies (hqpkkt_q_bfgs_update): the damped BFGS update of every block of
        q_blocks(bsize) for the step ``s`` and the change ``y`` of the Lagrangian's gradient; ``gamma`` < 0 adapts the
        damping to the step length ``alpha``.  ``pattern``: the update on the stored entries alone, any pattern (with
        bsize = 0 the update of Hqp_HL_Gangster); otherwise every block must be fully stored (HQPKKT_E_FORMAT).  Returns
        (v, Qs) - v as applied and the block-restricted Q s, None for the one not wanted.  q_bfgs_report() tells what every
        block did.  ``eigen_control``: the reference's _eps - the update is followed by q_eigen_control(eps, bsize,
        from_bfgs=True), the reference's default (sqp_hela_eigen_control); q_eigen_report() tells what that did."""
        ps, ks = self._vec_in(s, self.n, "s")
        py, ky = self._vec_in(y, self.n, "y")
        u = _lib.QBfgsUpdate()
        u.s, u.y, u.gamma, u.alpha, u.bsize = ps.value, py.value, float(gamma), float(alpha), int(bsize)
        u.fill = _lib.HQPKKT_QBFGS_PATTERN if pattern else _lib.HQPKKT_QBFGS_FULL
        v = Qs = None
        if want_v:
            pv, v = self._vec_out(self.n)
            u.v = pv.value
        if want_Qs:
            pq, Qs = self._vec_out(self.n)
            u.Qs = pq.value
        self._stream_sync()
        _check(self._L.hqpkkt_q_bfgs_update(self._h, C.byref(u)), "q_bfgs_update")
        self._keep_qv = [ks, ky, v, Qs]
        if want_v or want_Qs:
            self._stream_sync(after=True)
        if eigen_control is not None:
            self.q_eigen_control(eigen_control, bsize=bsize, from_bfgs=True)
        return v, Qs

    def q_eigen_control(self, eps, bsize=-1, from_bfgs=False, floor=None, max_steps=0):
        """The eigenvalue control of Hqp_HL_BFGS on the blocks of q_blocks(bsize) of the sparse Q where it lies
        (hqpkkt_q_eigen_control): every block whose smallest eigenvalue - estimated from below by a Lanczos recurrence on
        the device - lies under its floor gets the difference added to its diagonal.  The floor is eps^2; ``from_bfgs``
        lowers it to the s'Qs of the last q_bfgs_update() with this bsize where 0 <= s'Qs < eps^2 and skips the blocks that
        update left alone; ``floor`` (one value per block) overrides both.  ``max_steps``: 1 .. 128 Lanczos steps, 0 = 64.
        q_eigen_report() tells what every block did."""
        e = _lib.QEigenControl()
        e.eps, e.bsize, e.floor_from_bfgs, e.max_steps = float(eps), int(bsize), int(from_bfgs), int(max_steps)
        fl = None
        if floor is not None:
            fl = np.ascontiguousarray(floor, dtype=np.float64)
            k = C.c_longlong()
            _check(self._L.hqpkkt_q_blocks(self._h, int(bsize), None, None, 0, C.byref(k)), "q_blocks")
            if fl.shape != (k.value,):
                raise ValueError("q_eigen_control: floor holds one value per block of q_blocks(bsize)")
            e.floor = fl.ctypes.data
        self._stream_sync()
        _check(self._L.hqpkkt_q_eigen_control(self._h, C.byref(e)), "q_eigen_control")

    def q_eigen_report(self, with_T=False):
        """Per block of the last q_eigen_control() (hqpkkt_q_eigen_report), an array of shape (blocks, 10): Gerschgorin's bound
        g, the floor theta as used, the Lanczos steps, lo, hi (the bracket of T's smallest eigenvalue), rho (the residual
        bound), lambda_est = lo - rho, the shift d, |T| and the outcome - 0 no shift, by Gerschgorin; 1 no shift, by Lanczos;
        2 shifted, converged; 3 shifted, not converged; 4 left alone, not finite; 6 skipped, the last BFGS update left the
        block alone.  ``with_T``: returns (report, T), T of shape (blocks, 2, t_steps) - alpha then beta of the recurrence,
        t_steps the step cap of that control.  Waits for the handle's stream."""
        k, ts = C.c_longlong(), C.c_int()
        out = np.zeros((1, _lib.HQPKKT_EIG_REPORT))
        e = self._L.hqpkkt_q_eigen_report(self._h, C.c_void_p(out.ctypes.data), None, 0, C.byref(k), C.byref(ts))
        T = None
        if e in (0, _lib.E_RANGE):
            out = np.zeros((k.value, _lib.HQPKKT_EIG_REPORT))
            T = np.zeros((k.value, 2, ts.value)) if with_T else None
            e = self._L.hqpkkt_q_eigen_report(self._h, C.c_void_p(out.ctypes.data), C.c_void_p(T.ctypes.data) if with_T else None, k.value,
                                              C.byref(k), C.byref(ts))
        _check(e, "q_eigen_report")
        return (out, T) if with_T else out

    def q_bfgs_report(self):
        """Per block of the last q_bfgs_update() (hqpkkt_q_bfgs_report), an array of shape (blocks, 8): sy, sQs, gamma_eff,
        theta (1 where not damped), sv as used, first index, length and the outcome - 0 updated, 1 updated with damping,
        2 left alone (sv or sQs is zero), 3 left alone (sv or sQs is not finite).  Waits for the handle's stream."""
        k = C.c_longlong()
        out = np.zeros((1, _lib.HQPKKT_QBFGS_REPORT))
        e = self._L.hqpkkt_q_bfgs_report(self._h, C.c_void_p(out.ctypes.data), 1, C.byref(k))
        if e == _lib.E_RANGE:
            out = np.zeros((k.value, _lib.HQPKKT_QBFGS_REPORT))
            e = self._L.hqpkkt_q_bfgs_report(self._h, C.c_void_p(out.ctypes.data), k.value, C.byref(k))
        _check(e, "q_bfgs_report")
        return out[: k.value]

    def lagrangian_gradient(self, c, y, z, minus=None):
        """Hqp_SqpSolver::grd_L (hqpkkt_lagrangian_gradient): c - A'y - C'z, and minus ``minus`` where given - the
        difference of two gradients from the second call."""
        pc, kc = self._vec_in(c, self.n, "c")
        py, ky = self._vec_in(y if self.me else None, self.me, "y")
        pz, kz = self._vec_in(z if self.m else None, self.m, "z")
        pm, km = self._vec_in(minus, self.n, "minus")
        po, out = self._vec_out(self.n)
        self._stream_sync()
        _check(self._L.hqpkkt_lagrangian_gradient(self._h, pc, py, pz, pm, po), "lagrangian_gradient")
        self._stream_sync(after=True)
        return out

    def read_block(self, what, node):
        """Numeric block of a supernode after factor() (tests): 0 panel, 1 inverse of
        L11, 2 X, 3 update block; flat float64 array, column-major.  4 dinv (2 p), 5 ptype,
        6 lperm (p each, as float64), 7 the scale vector (dim, QP numbering; node unused)."""
        k = C.c_longlong()
        _check(self._L.hqpkkt_debug_read(self._h, what, node, None, 0, C.byref(k)), "debug_read")
        out = np.zeros(max(k.value, 1))
        _check(self._L.hqpkkt_debug_read(self._h, what, node, C.c_void_p(out.ctypes.data), k.value,
                                         C.byref(k)), "debug_read")
        return out[: k.value]

    def structure(self):
        names = ["elim", "piv_start", "npiv", "nborder", "parent", "level", "border_ptr",
                 "border_idx", "entry_row", "entry_col", "node_owner", "exchange_roots"]
        return {nm: self.debug(i) for i, nm in enumerate(names)}

    PLAN_HEADER = ("top_n", "top_lt", "top_lds", "top_ns", "small_tree", "tree_factor", "top_split", "tree_ldp", "tree_ldb",
                   "lds_panel", "lds_bwdb", "lds_blk", "nlevels", "record_ints", "nnodes0", "nnodes1")
    PLAN_RECORD = ("n", "nodes_off", "fs_n", "fs_ldp", "fs_ldb", "fs_lds", "sm_n", "sm_ldp", "sm_lds", "blk_n", "blk_inst",
                   "blk_threads", "blk_lds", "ps_grid", "ps_xps", "slabs_off", "su_n", "su_variant", "su_grid", "su_xsu", "tiles_off",
                   "big_n", "big_off", "fwd_form", "fwd_small_n", "fwd_grid", "fwd_a_grid", "gslabs_off", "bwd_small_n", "bwd_b_grid",
                   "bwd_a_grid", "cblks_off")
    FWD_NONE, FWD_ONE, FWD_AB, FWD_TOP, FWD_TREE = range(5)

    def launch_plan(self):
        """What this handle of the tree engine launches (hqpkkt_debug_get 48, csrc/tree_plan.hpp): the header's values by
        name and ``levels``: per schedule (this rank's subtrees, the replicated top) one dict per tree level.  After
        the analysis, with or without a device; before the upload it is the plan the environment gives now."""
        raw = [int(x) for x in self.debug(48)]
        plan = dict(zip(self.PLAN_HEADER, raw))
        assert plan["record_ints"] == len(self.PLAN_RECORD)
        h, r, nl = len(self.PLAN_HEADER), len(self.PLAN_RECORD), plan["nlevels"]
        plan["levels"] = [[dict(zip(self.PLAN_RECORD, raw[h + (w * nl + l) * r: h + (w * nl + l + 1) * r])) for l in range(nl)]
                          for w in range(2)]
        return plan


class Hqp_IpSpBKP(Hqp_IpMatrix):
    """Full (n+me+m) KKT system; semantics of hqp/Hqp_IpSpBKP.C."""
    _mode = _lib.MODE_FULL
    _name = "SpBKP"


class Hqp_IpRedSpBKP(Hqp_IpMatrix):
    """Reduced (n+me) system with C'ZW^-1C folded in; semantics of hqp/Hqp_IpRedSpBKP.C."""
    _mode = _lib.MODE_REDUCED
    _name = "RedSpBKP"


class Hqp_IpLQDOCP(Hqp_IpMatrix):
    """The multistage plugin hqp/Hqp_IpLQDOCP.C: stage structure found from the staircase of
    A (Get_Dim, :201-287), dense per-stage blocks, the extended Riccati recursion as fp64
    MFMA products (HQPKKT_MODE_STAGED).  ``set_stages(nx, nu)`` before init() gives the stage
    sizes explicitly.  ``a_sparse=True`` (the reference's mat_a_sparse, hqp/Hqp_IpLQDOCP.C:178) or
    ``set_dynamics_form("sparse")`` before init(): the stage products walk the row lists of A instead of
    dense blocks F_k - for dynamics with a few entries per column (hqpkkt_set_dynamics_form).  ``dense_columns=n``
    or ``set_dense_columns(n)`` with it: the columns of F_k with at least n entries go through the MFMA products as
    a small dense block (hqpkkt_set_dense_columns; -1: the library's threshold, 0: none).  ``a_profile=True`` or
    ``set_dynamics_form("profile")``: dense blocks F_k, the large products and the solve over the k-slabs that hold each
    128-column panel's stored entries - for banded and block-banded dynamics (HQPKKT_DYN_PROFILE).  ``a_packed=True`` or
    ``set_packed_panels(True)`` with it: the stages that run the profile sequence store F_k as packed panels, the rows of
    every panel's range alone (hqpkkt_set_packed_panels).  ``dense_rows=n`` or ``set_dense_rows(n)``, with any form of
    the dynamics: the rows of C with at least n entries leave the H term lists and go through the MFMA product as a
    dense block per stage, and step() and residuum() take them through the same block (hqpkkt_set_dense_rows; 0: none;
    dense_row_products() reports the split).  ``q_dense=True`` or ``set_hessian_form("dense")``, with any
    form of the dynamics: the stage Hessians Q_k are kept as dense blocks instead of entries of the H term lists
    (hqpkkt_set_hessian_form); init() scatters the CSR values into them, init_dense() takes ``DenseDocp.Qd``.
    ``q_packed=True`` or ``set_packed_hessians(True)`` with it: the blocks are stored as their 128 x 128 tiles on and below
    the diagonal wherever that is smaller (hqpkkt_set_packed_hessians; hessian_packing() reports the layout).
    After a dense hand-over the blocks live on the device: update_stage_hessians() changes them in place (scale, diagonal,
    up to four rank-one terms per stage), hessian_product() gives Q x, and bfgs_update() is the reference's damped block-BFGS
    step made of the two (hqpkkt_update_stage_hessians, hqpkkt_hessian_product) with its terms formed on the host;
    bfgs_update_device() forms them on the device too (hqpkkt_bfgs_update_stage_hessians), bfgs_report() reads what it did."""
    _mode = _lib.MODE_STAGED
    _name = "LQDOCP"

    def __init__(self, *args, a_sparse=False, dense_columns=0, a_profile=False, a_packed=False, dense_rows=0, q_dense=False, q_packed=False, **kw):
        super().__init__(*args, **kw)
        if q_packed:
            self.set_packed_hessians(True)
        if q_dense:
            self.set_hessian_form("dense")
        if a_sparse:
            self.set_dynamics_form("sparse")
        if a_profile:
            self.set_dynamics_form("profile")
        if dense_columns:
            self.set_dense_columns(dense_columns)
        if a_packed:
            self.set_packed_panels(True)
        if dense_rows:
            self.set_dense_rows(dense_rows)

    def set_dynamics_form(self, form):
        """"dense" (default), "sparse" or "profile"; holds from the next init() on."""
        code = {"dense": _lib.DYN_DENSE, "sparse": _lib.DYN_SPARSE, "profile": _lib.DYN_PROFILE}.get(form, form)
        _check(self._L.hqpkkt_set_dynamics_form(self._h, int(code)), "set_dynamics_form")

    def set_dense_columns(self, min_entries):
        """Columns of F_k with at least ``min_entries`` entries are heavy (sparse form; holds from the next init() on)."""
        _check(self._L.hqpkkt_set_dense_columns(self._h, int(min_entries)), "set_dense_columns")

    def dense_columns(self):
        """Per stage k < K the heavy columns, local to the stage (states, then controls), ascending; [] unless the
        sparse form is set."""
        d = self.debug(39)
        if d.size == 0:
            return []
        K = len(self.debug(21))
        ptr, cols = d[: K + 1], d[K + 1:]
        return [cols[ptr[k]: ptr[k + 1]].tolist() for k in range(K)]

    def set_dense_rows(self, min_entries):
        """Rows of C with at least ``min_entries`` entries are wide (holds from the next init() on)."""
        _check(self._L.hqpkkt_set_dense_rows(self._h, int(min_entries)), "set_dense_rows")

    def dense_rows(self):
        """Per stage k = 0 .. K the wide rows of C (row indices of C, ascending); [] unless the analysis had a threshold."""
        d = self.debug(43)
        if d.size == 0:
            return []
        K = len(self.debug(21))
        ptr, rows = d[: K + 2], d[K + 2:]
        return [rows[ptr[k]: ptr[k + 1]].tolist() for k in range(K + 1)]

    def dense_row_products(self):
        """How step() and residuum() take the wide rows of C (hqpkkt_debug_get 46): {"on": they go through the dense
        blocks E_k, "rows": wide rows, "kept": stored entries of C left to the CSR walks, "removed": entries the blocks
        hold instead}; {} unless the analysis found wide rows."""
        d = self.debug(46).astype(np.int64)
        if d.size == 0:
            return {}
        c = (d[2::2] & 0xFFFFFFFF) | (d[3::2] << 32)
        return {"on": bool(d[0]), "rows": int(d[1]), "kept": int(c[0]), "removed": int(c[1])}

    def h_terms(self):
        """(kept, removed): per stage k = 0 .. K the H terms in the plan's lists and the terms the stage's wide rows
        would have added, as int64 arrays; ([], []) unless the analysis had a threshold."""
        d = self.debug(43)
        if d.size == 0:
            return [], []
        K = len(self.debug(21))
        c = d[K + 2 + d[K + 1]:].astype(np.int64).reshape(K + 1, 2, 2)
        c = (c[..., 0] & 0xFFFFFFFF) | (c[..., 1] << 32)
        return c[:, 0].copy(), c[:, 1].copy()

    def dynamics_entries(self):
        """Per stage k < K: (stored entries of F_k, 1 where the stage runs the sparse sequence, 2 the profile sequence)."""
        return self.debug(36).reshape(-1, 2)

    def profile_ranges(self):
        """Per stage k < K the (lo, hi) k-slab ranges of the 128-column panels of F_k, an int array of shape (panels, 2);
        [] unless the profile form is set."""
        d = self.debug(41)
        if d.size == 0:
            return []
        K = len(self.debug(21))
        ptr, rng = d[: K + 1], d[K + 1:].reshape(-1, 2)
        return [rng[ptr[k]: ptr[k + 1]].copy() for k in range(K)]

    def set_hessian_form(self, form):
        """"csr" (default: term lists) or "dense" (a dense block Q_k per stage); holds from the next init() on."""
        code = {"csr": _lib.HESS_CSR, "dense": _lib.HESS_DENSE}.get(form, form)
        _check(self._L.hqpkkt_set_hessian_form(self._h, int(code)), "set_hessian_form")

    def hessian_layout(self):
        """Per stage k = 0 .. K (order of Q_k, leading dimension, H terms left in the lists), an int64 array of shape
        (K + 1, 3); [] unless the dense form of the Hessians is set."""
        d = self.debug(45)
        if d.size == 0:
            return []
        d = d.astype(np.int64).reshape(-1, 4)
        return np.stack([d[:, 0], d[:, 1], (d[:, 2] & 0xFFFFFFFF) | (d[:, 3] << 32)], axis=1)

    def set_stage_hessian(self, k, Q):
        """Block k of the dense Hessians (dense hand-over): a row-major matrix of which the entries j >= i are read; a
        numpy array, or a torch CUDA tensor with device_vectors=True."""
        if hasattr(Q, "data_ptr"):
            if not self._device_vectors or Q.stride(1) != 1:
                raise TypeError("Q blocks: row-major torch CUDA tensors need device_vectors=True")
            ptr, ld, keep = Q.data_ptr(), Q.stride(0), None  # (a device block is the caller's to keep until the stream has read it)
        else:
            if self._device_vectors:
                raise TypeError("device_vectors=True needs torch CUDA Q blocks")
            keep = np.ascontiguousarray(Q, dtype=np.float64)
            ptr, ld = keep.ctypes.data, keep.shape[1]
        _check(self._L.hqpkkt_set_stage_hessian(self._h, int(k), C.c_void_p(ptr), ld), "set_stage_hessian")
        # (the copy is asynchronous in the handle's stream: the block stays alive until the hand-over ends)
        if keep is not None:
            self._keep_q = getattr(self, "_keep_q", []) + [keep]

    def stage_hessian(self, k):
        """Q_k as it lies in the arena (tests): order x leading dimension, padding included."""
        n = C.c_longlong()
        _check(self._L.hqpkkt_debug_stage_hessian(self._h, k, None, 0, C.byref(n)), "stage_hessian")
        out = np.zeros(max(n.value, 1))
        _check(self._L.hqpkkt_debug_stage_hessian(self._h, k, C.c_void_p(out.ctypes.data), n.value, C.byref(n)), "stage_hessian")
        lay = self.hessian_layout()
        return out[: n.value].reshape(int(lay[k][0]), int(lay[k][1]))

    def hess_symv(self, x):
        """y = Q x over the dense stage Hessians by the kernel of the residual products (tests); x of length n."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.n
        y = np.zeros(self.n)
        _check(self._L.hqpkkt_debug_hess_symv(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)), "hess_symv")
        return y

    def hess_symv_timed(self, x, reps):
        """(y, ms): y = Q x and the average device time in ms of ``reps`` such products as the residual launches them."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.n
        y, ms = np.zeros(self.n), C.c_double()
        _check(self._L.hqpkkt_debug_hess_symv_timed(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), int(reps), C.byref(ms)),
               "hess_symv_timed")
        return y, ms.value

    def hessian_product(self, x):
        """y = Q x over the dense stage Hessians (hqpkkt_hessian_product): x of length n, numpy - or a torch CUDA tensor with
        device_vectors=True, and y is one then.  The launches and the bits of the residual's product."""
        px, kx = self._vec_in(x, self.n, "x")
        py, y = self._vec_out(self.n)
        self._stream_sync()
        _check(self._L.hqpkkt_hessian_product(self._h, px, py), "hessian_product")
        return y

    def update_stage_hessians(self, U, coef, beta=None, diag=None):
        """Every stage Hessian updated in place on the device (hqpkkt_update_stage_hessians):
        Q_k <- beta_k Q_k + diag(d_k) + sum_j coef[k, j] u_jk u_jk'.  ``U``: a list of r <= 4 vectors of n, ``diag``: a
        vector of n or None - numpy, or torch CUDA tensors with device_vectors=True (read asynchronously: they are kept
        alive here until the next call); ``coef``: host array of shape (K + 1, r); ``beta``: K + 1 host values or None
        (all 1).  beta_k = 0 makes block k on the device - ``diag`` alone is a scaled identity -, and a diagonal shift is
        ``diag`` with beta = 1.  The reference's restart and eigenvalue control, which read the blocks, are
        restart_hessians() and eigen_control()."""
        U = list(U)
        r = len(U)
        K1 = len(self.debug(20))
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(K1, r)
        keep = [coef]
        up = (C.c_void_p * max(r, 1))()
        for j, v in enumerate(U):
            p, k = self._vec_in(v, self.n, f"U[{j}]")
            up[j] = p.value
            keep.append(k)
        u = _lib.HessUpdate()
        u.r = r
        u.U = C.cast(up, C.POINTER(C.c_void_p)) if r else None
        u.coef = coef.ctypes.data if r else None
        if beta is not None:
            beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(K1)
            u.beta = beta.ctypes.data
        if diag is not None:
            p, k = self._vec_in(diag, self.n, "diag")
            u.diag = p.value
            keep.append(k)
        self._stream_sync()
        _check(self._L.hqpkkt_update_stage_hessians(self._h, C.byref(u)), "update_stage_hessians")
        self._keep_u = keep

    def bfgs_update(self, s, y, gamma=0.1, alpha=1.0):
        """The reference's damped BFGS update of every stage Hessian (Hqp_HL_BFGS::update_b_Q without its eigenvalue
        control) for the step ``s`` and the change ``y`` of the Lagrangian's gradient, numpy vectors of n: Q s by
        hessian_product, the terms by hessian_update.bfgs_terms on the host, the rank-2 update on the device.  Returns
        (U, coef) as applied."""
        from .hessian_update import bfgs_terms
        lay = self.hessian_layout()
        offsets = np.concatenate([[0], np.cumsum(lay[:, 0])])
        s = np.ascontiguousarray(s, dtype=np.float64)
        if self._device_vectors:
            import torch
            dev = torch.device("cuda", self._dev)
            Qs = self.hessian_product(torch.as_tensor(s).to(dev)).cpu().numpy()
            U, coef = bfgs_terms(s, y, Qs, offsets, gamma, alpha)
            self.update_stage_hessians([torch.as_tensor(v).to(dev) for v in U], coef)
        else:
            U, coef = bfgs_terms(s, y, self.hessian_product(s), offsets, gamma, alpha)
            self.update_stage_hessians(U, coef)
        return U, coef

    def bfgs_update_device(self, s, y, gamma=0.1, alpha=1.0, want_v=False, eigen_control=None):
        """The same update with its terms formed on the device as well (hqpkkt_bfgs_update_stage_hessians): Q s, the
        scalars, Powell's test, v and the coefficients never reach the host.  ``s``, ``y``: numpy vectors of n - or torch
        CUDA tensors with device_vectors=True: no host copy is made, the call returns with the work enqueued in the
        handle's stream, and the tensors are kept alive here until the next call.  ``gamma`` < 0: damping adapted to the
        step length ``alpha``.  ``want_v``: returns v as applied (a tensor with device_vectors=True), else None.
        ``eigen_control``: an eps - the reference's eigenvalue control runs behind the update in the same stream,
        eigen_control(eps, from_bfgs=True); None (the default): the update alone.  bfgs_report() tells what every stage did."""
        ps, ks = self._vec_in(s, self.n, "s")
        py, ky = self._vec_in(y, self.n, "y")
        b = _lib.BfgsUpdate()
        b.s, b.y, b.gamma, b.alpha = ps.value, py.value, float(gamma), float(alpha)
        v = None
        if want_v:
            pv, v = self._vec_out(self.n)
            b.v = pv.value
        self._stream_sync()
        _check(self._L.hqpkkt_bfgs_update_stage_hessians(self._h, C.byref(b)), "bfgs_update_device")
        self._keep_b = [ks, ky, v]
        if eigen_control is not None:
            self.eigen_control(eigen_control, from_bfgs=True)
        return v

    def bfgs_report(self):
        """Per stage k = 0 .. K what the last bfgs_update_device() did (hqpkkt_bfgs_report), an array of shape (K + 1, 8):
        s'y, s'Qs, the damping factor used, theta (1 where not damped), s'v as used, the coefficients 1 / s'v and
        -1 / s'Qs (0 where the stage was left alone), and the outcome - 0 updated, 1 updated with damping, 2 left alone
        (s'v or s'Qs is zero), 3 left alone (s'v or s'Qs is not finite).  Waits for the handle's stream."""
        out = np.zeros((len(self.debug(20)), _lib.HQPKKT_BFGS_REPORT))
        _check(self._L.hqpkkt_bfgs_report(self._h, C.c_void_p(out.ctypes.data)), "bfgs_report")
        return out

    def hessian_row_stats(self, want_max=True, want_sum=True):
        """(rowmax, offsum) of every stage Hessian (hqpkkt_hessian_row_stats): per variable i of stage k the largest
        |Q_k(i, j)| and the sum of |Q_k(i, j)| over j != i, vectors of n - numpy, or torch CUDA tensors with
        device_vectors=True.  The entry writes device vectors asynchronously in the handle's stream, which torch's streams do
        not wait for: this wrapper waits for the device before it returns the tensors.  None for the one not wanted."""
        out = [self._vec_out(self.n) if w else (None, None) for w in (want_max, want_sum)]
        self._stream_sync()
        _check(self._L.hqpkkt_hessian_row_stats(self._h, out[0][0], out[1][0]), "hessian_row_stats")
        self._stream_sync(after=True)
        return out[0][1], out[1][1]

    def restart_hessians(self, eps, stages=None):
        """The reference's restart_Q on the device (hqpkkt_restart_stage_hessians): Q_k <- diag(min(max(eps, rowmax_i),
        1 / eps)) on the stages whose entry of ``stages`` (K + 1 flags) is set; None: on all."""
        flags = None
        if stages is not None:
            flags = np.ascontiguousarray(np.asarray(stages) != 0, dtype=np.uint8).reshape(len(self.debug(20)))
        _check(self._L.hqpkkt_restart_stage_hessians(self._h, float(eps), None if flags is None else C.c_void_p(flags.ctypes.data)), "restart_hessians")

    def gerschgorin_hessians(self, eps):
        """Hqp_HL_Gerschgorin::update on the device (hqpkkt_gerschgorin_stage_hessians): q_ii <- max(q_ii, sum_{j != i}
        |q_ij| + eps) on every stage; the diagonal entries alone are written."""
        _check(self._L.hqpkkt_gerschgorin_stage_hessians(self._h, float(eps)), "gerschgorin_hessians")

    def eigen_control(self, eps, floor=None, from_bfgs=False, max_steps=0):
        """The eigenvalue control of Hqp_HL_BFGS::update_b_Q on the device (hqpkkt_eigen_control_stage_hessians): every
        stage whose smallest eigenvalue, estimated from below by a Lanczos recurrence over all stages, lies under its
        floor theta_k gets its diagonal shifted up by the difference.  theta_k = eps^2; ``from_bfgs``: lowered to s'Qs of
        the last bfgs_update_device() where 0 <= s'Qs < eps^2 (the reference's rule, read on the device); ``floor``: K + 1
        host values that override both.  ``max_steps``: 1 .. 128 Lanczos steps, 0: 64.  The call returns with the work
        enqueued; eigen_report() tells what every stage did."""
        c = _lib.EigenControl()
        c.eps, c.floor_from_bfgs, c.max_steps = float(eps), int(bool(from_bfgs)), int(max_steps)
        if floor is not None:
            floor = np.ascontiguousarray(floor, dtype=np.float64).reshape(len(self.debug(20)))
            c.floor = floor.ctypes.data
        _check(self._L.hqpkkt_eigen_control_stage_hessians(self._h, C.byref(c)), "eigen_control")

    def eigen_report(self, with_T=False):
        """Per stage k = 0 .. K what the last eigen_control() did (hqpkkt_eigen_report), an array of shape (K + 1, 10):
        Gerschgorin's bound g_k, the floor theta_k as used, the Lanczos steps, the bracket lo, hi of the smallest Ritz
        value, the residual bound rho, the estimate lo - rho, the shift d_k, |T| and the outcome - 0 no shift by
        Gerschgorin, 1 no shift by Lanczos, 2 shifted and converged, 3 shifted and not converged, 4 left alone (not
        finite), 5 order 0.  ``with_T``: (report, T) with T of shape (K + 1, 2, 128), alpha then beta of every stage.
        Waits for the handle's stream."""
        K1 = len(self.debug(20))
        out = np.zeros((K1, _lib.HQPKKT_EIG_REPORT))
        T = np.zeros((K1, 2, _lib.HQPKKT_EIG_MAX_STEPS)) if with_T else None
        _check(self._L.hqpkkt_eigen_report(self._h, C.c_void_p(out.ctypes.data), None if T is None else C.c_void_p(T.ctypes.data)), "eigen_report")
        return (out, T) if with_T else out

    def set_packed_hessians(self, on):
        """Dense stage Hessians stored as packed lower tiles (hqpkkt_set_packed_hessians); holds from the next init() on."""
        _check(self._L.hqpkkt_set_packed_hessians(self._h, int(on)), "set_packed_hessians")

    def hessian_packing(self):
        """Per stage k = 0 .. K (tile edge or 0 where the stage keeps its dense block, tiles stored, arena elements, doubles
        one dense hand-over moves from the caller's host block, doubles of the product's scratch), an int64 array of shape
        (K + 1, 5); [] unless packing was analysed with the dense form of the Hessians."""
        d = self.debug(47)
        if d.size == 0:
            return []
        d = d.astype(np.int64).reshape(-1, 8)
        c = (d[:, 2::2] & 0xFFFFFFFF) | (d[:, 3::2] << 32)
        return np.concatenate([d[:, :2], c], axis=1)

    def set_packed_panels(self, on):
        """Packed panels of the profile form (hqpkkt_set_packed_panels); holds from the next init() on."""
        _check(self._L.hqpkkt_set_packed_panels(self._h, int(on)), "set_packed_panels")

    def packed_panels(self):
        """Per stage k < K an int array of shape (panels, 2): per 128-column panel of F_k its offset in doubles from the
        stage's first panel and its leading dimension, (-1, 0) where the stage keeps its dense block; [] unless the
        profile form is set."""
        d = self.debug(42)
        if d.size == 0:
            return []
        K = len(self.debug(21))
        ptr, pan = d[: K + 1], d[K + 1:].reshape(-1, 2)
        return [pan[ptr[k]: ptr[k + 1]].copy() for k in range(K)]

    def set_stages(self, nx, nu):
        nx, nu = _i32(nx), _i32(nu)
        _check(self._L.hqpkkt_set_stages(self._h, len(nu), C.c_void_p(nx.ctypes.data),
                                         C.c_void_p(nu.ctypes.data) if nu.size else None), "set_stages")

    def init_dense(self, dq):
        """init() for a :class:`hqp_amd.problems.DenseDocp`: the dynamics as dense blocks
        (hqpkkt_analyze_staged + hqpkkt_set_values_staged)."""
        self.n, self.me, self.m = dq.dims
        nx, nu = _i32(dq.nx), _i32(dq.nu)
        arrs = []
        qd = getattr(dq, "Qd", None) is not None  # (dense stage Hessians: Q's pattern is not read)
        empty = (np.zeros(0, dtype=np.int32),) * 3
        for (p, i, _x) in (empty if qd else dq.Q, dq.E, dq.C):
            arrs += [_i32(p), _i32(i)]
        self._keep = arrs + [nx, nu]
        ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
        _check(self._L.hqpkkt_analyze_staged(self._h, dq.K, C.c_void_p(nx.ctypes.data), C.c_void_p(nu.ctypes.data),
                                             dq.n, dq.me_rest, dq.m, *ptrs), "init_dense")
        self.update_dense(dq)

    def update_dense(self, dq):
        vals, keep = [], []
        qd = getattr(dq, "Qd", None)
        if qd is not None:  # the blocks Q_k first; the values of Q's CSR form are not read
            assert len(qd) == dq.K + 1
            self._keep_q = []
            for k, blk in enumerate(qd):
                self.set_stage_hessian(k, blk)
        for (_p, _i, x) in ((None, None, np.zeros(0)) if qd is not None else dq.Q, dq.E, dq.C):
            if self._device_vectors and not hasattr(x, "data_ptr"):
                import torch
                x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()
            if hasattr(x, "data_ptr"):
                keep.append(x)
                vals.append(C.c_void_p(x.data_ptr()) if x.numel() else None)
            else:
                a = np.ascontiguousarray(x, dtype=np.float64)
                keep.append(a)
                vals.append(C.c_void_p(a.ctypes.data) if a.size else None)
        fp = (C.c_void_p * dq.K)()
        ld = (C.c_longlong * dq.K)()
        for k, blk in enumerate(dq.F):
            if hasattr(blk, "data_ptr"):
                if not self._device_vectors or blk.stride(1) != 1:
                    raise TypeError("F blocks: row-major torch CUDA tensors need device_vectors=True")
                fp[k], ld[k] = blk.data_ptr(), blk.stride(0)
                keep.append(blk)
            else:
                if self._device_vectors:
                    raise TypeError("device_vectors=True needs torch CUDA F blocks")
                a = np.ascontiguousarray(blk, dtype=np.float64)
                fp[k], ld[k] = a.ctypes.data, a.shape[1]
                keep.append(a)
        _check(self._L.hqpkkt_set_values_staged(self._h, vals[0], fp, ld, vals[1], vals[2]), "update_dense")
        self._keep_q = []  # (set_values_staged has waited for the stream)

    def lagrangian_gradient_staged(self, c, y, z, minus=None):
        """Hqp_SqpSolver::grd_L on a handle of the dense hand-over (hqpkkt_lagrangian_gradient_staged): c - A'y - C'z with
        the dynamics rows of A read from the blocks F_k on the device, and minus ``minus`` where given - the difference of
        two gradients from the second call, the y of bfgs_update_device().  ``y`` in the reference's row order: the
        dynamics rows first, then the rows of E.  numpy vectors, or torch CUDA tensors with device_vectors=True."""
        pc, kc = self._vec_in(c, self.n, "c")
        py, ky = self._vec_in(y if self.me else None, self.me, "y")
        pz, kz = self._vec_in(z if self.m else None, self.m, "z")
        pm, km = self._vec_in(minus, self.n, "minus")
        po, out = self._vec_out(self.n)
        self._stream_sync()
        _check(self._L.hqpkkt_lagrangian_gradient_staged(self._h, pc, py, pz, pm, po), "lagrangian_gradient_staged")
        self._stream_sync(after=True)
        return out

    def stage_structure(self):
        names = {"nk": 20, "mk": 21, "nmk": 22, "eq_ptr": 23, "eq_rows": 24, "fix_rows": 25, "cap": 26}
        return {nm: self.debug(i) for nm, i in names.items()}

    def stage_block(self, k):
        """V_k of the last factorisation (tests)."""
        n = C.c_longlong()
        _check(self._L.hqpkkt_debug_stage_block(self._h, k, None, 0, C.byref(n)), "stage_block")
        out = np.zeros(max(n.value, 1))
        _check(self._L.hqpkkt_debug_stage_block(self._h, k, C.c_void_p(out.ctypes.data), n.value, C.byref(n)), "stage_block")
        nk = int(round(n.value ** 0.5))
        return out[: n.value].reshape(nk, nk)

    def stages_fused(self):
        """Per stage whether V_k comes out of the G_xx launch (HQPKKT_FUSED_V)."""
        return self.debug(35)

    def ctrl_rows(self):
        """(W launches that fell back to the thin product since the upload, per stage whether the W launch takes the
        control-row segment)."""
        d = self.debug(44)
        return int(d[0]), d[1:]

    def stage_ranks(self):
        """(rank, carried rows) per stage of the last factorisation (tests)."""
        K1 = len(self.debug(20))
        out = np.zeros(2 * K1, dtype=np.int32)
        _check(self._L.hqpkkt_debug_stage_ranks(self._h, C.c_void_p(out.ctypes.data), out.size), "stage_ranks")
        return out.reshape(K1, 2)


class Hqp_IpLQDOCPFull(Hqp_IpMatrix):
    """The same KKT system under the plugin name LQDOCP solved by the full-system engine
    (the band ordering carries the stage structure): the comparison partner of the STAGED
    engine, and what the reference-side shim falls back to for QPs whose stages the STAGED
    kernels do not hold."""
    _mode = _lib.MODE_FULL
    _name = "LQDOCP"


IpSpBKP = Hqp_IpSpBKP
IpRedSpBKP = Hqp_IpRedSpBKP
IpLQDOCP = Hqp_IpLQDOCP
IpLQDOCPFull = Hqp_IpLQDOCPFull


def bench_dgemm(M, N, K, lower=False, mirror=False, reps=5, device=0):
    """(ms per launch, TFLOP/s, max relative error) of the STAGED engine's fp64 MFMA product."""
    ms, err = C.c_double(), C.c_double()
    _check(_lib.lib().hqpkkt_debug_dgemm(device, M, N, K, int(lower), int(mirror), reps, C.byref(ms), C.byref(err)), "debug_dgemm")
    flops = (1.0 if lower else 2.0) * M * N * K
    return ms.value, flops / (ms.value * 1e-3) / 1e12, err.value


def bench_dgemm2(M, N, K, K2, lower=True, mirror=True, reps=1, device=0):
    """The product with a second k segment, C = A'B - A2'B2 out of one launch: (ms per launch, max relative error, entries of
    a mirrored result that differ in a bit from their image)."""
    ms, err, asym = C.c_double(), C.c_double(), C.c_longlong()
    _check(_lib.lib().hqpkkt_debug_dgemm2(device, M, N, K, K2, int(lower), int(mirror), reps, C.byref(ms), C.byref(err), C.byref(asym)), "debug_dgemm2")
    return ms.value, err.value, asym.value


def dgemm_full(M, N, K, C_buf, c_row0, c_col0, A=None, a_col0=0, B=None, b_col0=0, alpha=1.0, beta=0.0, Cin=None, cin_col0=0,
               cin_is_c=False, lower=False, mirror=False, K2=0, A2=None, a2_col0=0, B2=None, b2_col0=0,
               sharded=False, no_ks=False, no_tile_map=False, force_split=False, device=0, krange=None, krange_by=0, packed=None, panel=None):
    """One launch of the STAGED engine's fp64 product on the caller's operands (hqpkkt_debug_dgemm_full): C_buf's block at
    (c_row0, c_col0) = alpha (A'B + A2'B2) + beta Cin.  Every array is a C-contiguous float64 matrix, rows x leading
    dimension; an operand's block starts at its column *_col0 and its rows behind K (K2) are the caller's to poison.
    C_buf is overwritten with the whole device buffer after the launch.  Returns (form, tiles, tile order used, operands
    staged by LDS-DMA, pieces of k).  krange with krange_by 1 / 2: the profile form - (lo, hi) k-slabs per 128-wide column
    panel of B / of A; the form comes back as "profile"."""
    import numpy as np

    def operand(x, col0):
        if x is None:
            return _lib.DgemmOperand(None, 0, 0, 0)
        assert x.dtype == np.float64 and x.ndim == 2 and x.flags.c_contiguous
        return _lib.DgemmOperand(x.ctypes.data, x.shape[0], x.shape[1], col0)

    assert C_buf.dtype == np.float64 and C_buf.ndim == 2 and C_buf.flags.c_contiguous and C_buf.flags.writeable
    c = _lib.DgemmCase()
    c.M, c.N, c.K, c.K2 = M, N, K, K2
    c.lower, c.mirror, c.cin_is_c = int(lower), int(mirror), int(cin_is_c)
    c.flags = sharded * 1 | no_ks * 8 | no_tile_map * 16 | force_split * 32
    c.alpha, c.beta = alpha, beta
    c.A, c.B, c.A2, c.B2, c.Cin = operand(A, a_col0), operand(B, b_col0), operand(A2, a2_col0), operand(B2, b2_col0), operand(Cin, cin_col0)
    c.C, c.c_rows, c.ldc, c.c_row0, c.c_col0 = C_buf.ctypes.data, C_buf.shape[0], C_buf.shape[1], c_row0, c_col0
    if krange_by:
        kr = np.ascontiguousarray(krange, dtype=np.int32)
        c.krange, c.krange_by = kr.ctypes.data, int(krange_by)
    if packed is not None:
        pk, pan = _packed_args(packed, panel)
        _check(_lib.lib().hqpkkt_debug_dgemm_packed(device, C.byref(c), pk.ctypes.data, pk.size, pan.ctypes.data), "debug_dgemm_packed")
    else:
        _check(_lib.lib().hqpkkt_debug_dgemm_full(device, C.byref(c)), "debug_dgemm_full")
    return (GEMM_FORMS + ("profile",))[c.form], c.tiles, bool(c.tile_map), bool(c.ldsdma), c.nsplit


def _packed_args(packed, panel):
    import numpy as np
    assert packed.dtype == np.float64 and packed.ndim == 1 and packed.flags.c_contiguous
    return packed, np.ascontiguousarray(panel, dtype=np.int64)


def dgemm_packed(M, N, K, C_buf, c_row0, c_col0, packed, panel, krange, krange_by, **kw):
    """:func:`dgemm_full` with the ranged operand (krange_by 1: B, 2: A) given as packed panels
    (hqpkkt_debug_dgemm_packed): ``packed`` a flat float64 buffer, ``panel`` (offset, ld) per 128-column panel of the
    operand, ``krange`` its (lo, hi) k-slabs.  The other operand and C_buf as in dgemm_full."""
    return dgemm_full(M, N, K, C_buf, c_row0, c_col0, krange=krange, krange_by=krange_by, packed=packed, panel=panel, **kw)


def gemv_packed(packed, panel, ranges, x, K, N, add=None, alpha=1.0, rows_form=False, y=None, device=0):
    """:func:`gemv_profile` on packed panels (hqpkkt_debug_gemv_packed): A is K x N, given as a flat float64 buffer and
    (offset, ld) per 128-column panel."""
    import numpy as np
    pk, pan = _packed_args(packed, panel)
    r = np.ascontiguousarray(ranges, dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    add = None if add is None else np.ascontiguousarray(add, dtype=np.float64)
    y = np.zeros(K if rows_form else N) if y is None else y
    assert x.size == (N if rows_form else K) and y.size == (K if rows_form else N) and r.size == 2 * ((N + 127) // 128) == pan.size
    _check(_lib.lib().hqpkkt_debug_gemv_packed(device, int(rows_form), K, N, pk.ctypes.data, pk.size, pan.ctypes.data, r.ctypes.data, x.ctypes.data,
                                               None if add is None else add.ctypes.data, float(alpha), y.ctypes.data), "debug_gemv_packed")
    return y


def carried_packed(BT, R, packed, panel, ranges, K, N, C_buf, c_row0, c_col0, device=0):
    """The carried rows of a packed stage (hqpkkt_debug_carried_packed, k_pk_carried): C_buf's block at (c_row0, c_col0)
    = BT[:K, :R]' F over every panel's range, F (K x N) given as packed panels.  BT and C_buf are C-contiguous float64
    matrices; C_buf is overwritten with the whole device buffer after the launch."""
    import numpy as np
    pk, pan = _packed_args(packed, panel)
    r = np.ascontiguousarray(ranges, dtype=np.int32)
    for a in (BT, C_buf):
        assert a.dtype == np.float64 and a.ndim == 2 and a.flags.c_contiguous
    assert r.size == 2 * ((N + 127) // 128) == pan.size
    _check(_lib.lib().hqpkkt_debug_carried_packed(device, K, N, R, BT.ctypes.data, BT.shape[0], BT.shape[1], pk.ctypes.data, pk.size, pan.ctypes.data,
                                                  r.ctypes.data, C_buf.ctypes.data, C_buf.shape[0], C_buf.shape[1], c_row0, c_col0), "debug_carried_packed")
    return C_buf


SK_KINDS = ("unequal", "equal", "frac")


def sk_table(tiles, nslab, grid=512, kind="unequal"):
    """A work list of the cut forms of the fp64 product (host only): (units[grid, stride, 6], pieces, whole_a, whole_b),
    a unit = (tile or -1, first k-slab, one past the last, first parking slot of the tile, pieces of the tile, piece).
    kind: unequal shares for the two workgroups of a CU, equal shares in rounds and phases, or the fractional cut."""
    import numpy as np
    k = SK_KINDS.index(kind)
    pieces, wa, wb = C.c_longlong(), C.c_int(), C.c_int()
    stride = _lib.lib().hqpkkt_debug_sk_table(tiles, nslab, grid, k, None, 0, C.byref(pieces), C.byref(wa), C.byref(wb))
    if stride <= 0:
        return None
    u = np.zeros((grid, stride, 6), dtype=np.int32)
    got = _lib.lib().hqpkkt_debug_sk_table(tiles, nslab, grid, k, u.ctypes.data_as(C.POINTER(C.c_int)), u.size, C.byref(pieces), C.byref(wa), C.byref(wb))
    assert got == stride
    return u, pieces.value, wa.value, wb.value


def sk_ctrl_rows(tiles_m, tiles_n, nslab, grid=512, kind=None):
    """The work list and tile order of a launch with the control-row segment (host only): (units[grid, stride, 6],
    tile_map[tiles_m tiles_n + 1], pieces) or None.  kind None: the list the engine's chooser gives; tile_map: logical tile
    -> tile row << 16 | tile column, negative: the augmented form."""
    import numpy as np
    k = -1 if kind is None else SK_KINDS.index(kind)
    pieces = C.c_longlong()
    stride = _lib.lib().hqpkkt_debug_sk_ctrl_rows(tiles_m, tiles_n, nslab, grid, k, None, 0, None, C.byref(pieces))
    if stride <= 0:
        return None
    u = np.zeros((grid, stride, 6), dtype=np.int32)
    m = np.zeros(tiles_m * tiles_n + 1, dtype=np.int32)
    got = _lib.lib().hqpkkt_debug_sk_ctrl_rows(tiles_m, tiles_n, nslab, grid, k, u.ctypes.data_as(C.POINTER(C.c_int)), u.size,
                                               m.ctypes.data_as(C.POINTER(C.c_int)), C.byref(pieces))
    assert got == stride
    return u, m, pieces.value


def dgemm_ctrl_rows(M, N, mu, A, B, C_buf, Cu_buf, grid=0, a_col0=0, b_col0=0, device=0):
    """One launch of C (M x N) = A'B (K = M) with the control-row segment for its last mu columns, and the guarded thin
    product behind it (hqpkkt_debug_dgemm_ctrl_rows): C_buf's block at (0, 0) and Cu_buf's first mu rows = C[:, N - mu:]'B.
    Both buffers are overwritten with the whole device buffers.  Returns (segment taken, fallbacks, form, tiles)."""
    import numpy as np
    for x in (A, B, C_buf, Cu_buf):
        assert x.dtype == np.float64 and x.ndim == 2 and x.flags.c_contiguous
    c = _lib.CtrlRowsCase()
    c.M, c.N, c.mu, c.grid = M, N, mu, grid
    c.A = _lib.DgemmOperand(A.ctypes.data, A.shape[0], A.shape[1], a_col0)
    c.B = _lib.DgemmOperand(B.ctypes.data, B.shape[0], B.shape[1], b_col0)
    c.C, c.c_rows, c.ldc = C_buf.ctypes.data, C_buf.shape[0], C_buf.shape[1]
    c.Cu, c.cu_rows, c.ldcu = Cu_buf.ctypes.data, Cu_buf.shape[0], Cu_buf.shape[1]
    _check(_lib.lib().hqpkkt_debug_dgemm_ctrl_rows(device, C.byref(c)), "debug_dgemm_ctrl_rows")
    return bool(c.taken), c.fallbacks, GEMM_FORMS[c.form], c.tiles


def sk_profile(ranges, grid=512):
    """The work list of the profile form (host only) for tiles of which tile t takes the k-slabs [ranges[t, 0],
    ranges[t, 1]): (units[grid, stride, 6], pieces), units as in :func:`sk_table`."""
    import numpy as np
    r = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
    rp, pieces = r.ctypes.data_as(C.POINTER(C.c_int)), C.c_longlong()
    stride = _lib.lib().hqpkkt_debug_sk_profile(rp, len(r), grid, None, 0, C.byref(pieces))
    if stride <= 0:
        return None
    u = np.zeros((grid, stride, 6), dtype=np.int32)
    got = _lib.lib().hqpkkt_debug_sk_profile(rp, len(r), grid, u.ctypes.data_as(C.POINTER(C.c_int)), u.size, C.byref(pieces))
    assert got == stride
    return u, pieces.value


def gemv_profile(A, ranges, x, add=None, alpha=1.0, rows_form=False, K=None, N=None, y=None, device=0):
    """One launch of a product of the profile form's solve (hqpkkt_debug_gemv_profile) on a C-contiguous float64 matrix A
    (rows x leading dimension, a multiple of 8): rows_form False: y (N) = add + alpha A[:K, :N]' x over the rows of every
    128-column panel's k-slab range; True: y (K) = add + alpha A[:K, :N] x over the panels whose range holds the row."""
    import numpy as np
    assert A.dtype == np.float64 and A.ndim == 2 and A.flags.c_contiguous
    K, N = A.shape[0] if K is None else K, A.shape[1] if N is None else N
    r = np.ascontiguousarray(ranges, dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    add = None if add is None else np.ascontiguousarray(add, dtype=np.float64)
    y = np.zeros(K if rows_form else N) if y is None else y
    assert x.size == (N if rows_form else K) and y.size == (K if rows_form else N) and r.size == 2 * ((N + 127) // 128)
    _check(_lib.lib().hqpkkt_debug_gemv_profile(device, int(rows_form), K, N, A.ctypes.data, A.shape[0], A.shape[1], r.ctypes.data, x.ctypes.data,
                                                None if add is None else add.ctypes.data, float(alpha), y.ctypes.data), "debug_gemv_profile")
    return y


GEMV_FORMS = ("rows", "wide", "cols")


def _gemv_case(A, M, N, x, ny, col0=0, add=None, scale=1.0, A2=None, a2_col0=0, n2=0, x2=None, add2=None, y=None, y2=None, part_chunks=1,
               xoff=0, yoff=0, own_x=True, own_y=True):
    """A hqpkkt_gemv_case over the caller's arrays and the arrays that must outlive the call: (case, y, y2, kept)."""
    import numpy as np

    def vec(v):
        return None if v is None else np.ascontiguousarray(v, dtype=np.float64)

    def operand(a, c0):
        if a is None:
            return _lib.DgemmOperand(None, 0, 0, 0)
        assert a.dtype == np.float64 and a.ndim == 2 and a.flags.c_contiguous
        return _lib.DgemmOperand(a.ctypes.data, a.shape[0], a.shape[1], c0)

    x, x2, add, add2 = vec(x), vec(x2), vec(add), vec(add2)
    if own_y and y is None:
        y = np.full(ny, np.nan)
    if add2 is not None and y2 is None:
        y2 = np.full(ny, np.nan)
    for v in (add, add2, y, y2):
        assert v is None or (v.dtype == np.float64 and v.size == ny and v.flags.c_contiguous)
    c = _lib.GemvCase()
    c.M, c.N, c.A, c.A2, c.n2, c.part_chunks = M, N, operand(A, col0), operand(A2, a2_col0), n2, part_chunks
    if own_x and x is not None:
        c.x, c.x_len = x.ctypes.data, x.size
    if x2 is not None:
        c.x2, c.x2_len = x2.ctypes.data, x2.size
    c.add = None if add is None else add.ctypes.data
    c.add2 = None if add2 is None else add2.ctypes.data
    c.scale, c.xoff, c.yoff = float(scale), xoff, yoff
    c.y = None if y is None else y.ctypes.data
    c.y2 = None if y2 is None else y2.ctypes.data
    return c, y, y2, (A, A2, x, x2, add, add2)


def gemv_dense(form, A, M, N, x, device=0, **kw):
    """One launch of a dense vector product of the STAGED solve (hqpkkt_debug_gemv_dense) on a C-contiguous float64
    matrix A (rows x leading dimension; the block starts at column col0).  form "rows" / "wide": y (M) = scale (add +
    A[:M, :N] x + A2[:M, :n2] x2) (A2 on the rows form alone); "cols": y (N) = add + scale A[:M, :N]' x, y2 = y + add2,
    part_chunks in place of the plan's.  x, x2 are uploaded whole.  Returns (y, y2 or None, chunks launched, rows - "cols":
    whether the block - that took the 16-byte loads)."""
    f = GEMV_FORMS.index(form)
    c, y, y2, _kept = _gemv_case(A, M, N, x, N if f == 2 else M, **kw)
    _check(_lib.lib().hqpkkt_debug_gemv_dense(device, f, C.byref(c)), "debug_gemv_dense")
    return y, y2, c.chunks, c.vec16


ROWS_GEMV_FORMS = ("rows", "rows_step", "cols")


def rows_gemv(form, blocks, E, row_index, n, m, x=None, t=None, tz=None, zw=None, r3=None, y=None, dz=None, dw=None, xc=None, device=0):
    """One launch of a vector product of the wide rows of C (hqpkkt_debug_rows_gemv) on the caller's arrays.  blocks: per
    block (rows, columns that count, leading dimension, offset into E, first entry of x of its column 0); E: float64, all
    blocks; row_index: per row of every block, in their order, its index into the m-vectors.  form "rows": y[row] = E_b[i]
    . x[col0:col0 + cols] (x: n, y: m); "rows_step": dz[row] = tz[row] - zw[row] cdx, dw[row] = -r3[row] + cdx; "cols":
    xc[col0 + c] = sum_i E_b[i][c] t[row of i] (t: m, xc: n).  Results start from the arrays given (NaN where none is) and
    keep every entry the launch does not own.  Returns y, (dz, dw) or xc."""
    import numpy as np
    f = ROWS_GEMV_FORMS.index(form)

    def vec(v, k, fill=None):
        if v is None:
            return None if fill is None else np.full(k, fill)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert v.size == k
        return v

    ints = [np.ascontiguousarray([b[q] for b in blocks], dtype=np.int32) for q in (0, 1, 2, 4)]
    off = np.ascontiguousarray([b[3] for b in blocks], dtype=np.int64)
    E = np.ascontiguousarray(E, dtype=np.float64).ravel()
    ri = np.ascontiguousarray(row_index, dtype=np.int32)
    assert ri.size == int(ints[0].sum())
    if ri.size == 0:
        ri = np.zeros(1, np.int32)
    x, t, tz, zw, r3 = vec(x, n), vec(t, m), vec(tz, m), vec(zw, m), vec(r3, m)
    out = {"y": vec(y, m, np.nan) if f == 0 else None, "dz": vec(dz, m, np.nan) if f == 1 else None, "dw": vec(dw, m, np.nan) if f == 1 else None,
           "xc": vec(xc, n, np.nan) if f == 2 else None}
    out = {k: (None if v is None else v.copy()) for k, v in out.items()}
    c = _lib.RowsCase()
    c.nblocks, c.e_len, c.n, c.m = len(blocks), E.size, n, m
    c.rows, c.cols, c.ld, c.col0 = (a.ctypes.data for a in ints)
    c.off, c.E, c.row_index = off.ctypes.data, E.ctypes.data, ri.ctypes.data
    for name, v in (("x", x), ("t", t), ("tz", tz), ("zw", zw), ("r3", r3), ("y", out["y"]), ("dz", out["dz"]), ("dw", out["dw"]), ("xc", out["xc"])):
        setattr(c, name, None if v is None else v.ctypes.data)
    _check(_lib.lib().hqpkkt_debug_rows_gemv(device, f, C.byref(c)), "debug_rows_gemv")
    return out["y"] if f == 0 else (out["dz"], out["dw"]) if f == 1 else out["xc"]


def symv(V, N, x, device=0, **kw):
    """y (N) = scale (add + V x + A2 x2) for a symmetric V by the triangle form (hqpkkt_debug_symv): only V's elements on
    and below the diagonal are read.  V: C-contiguous float64, even leading dimension, even col0.  Returns (y, tiles)."""
    c, y, _y2, _kept = _gemv_case(V, N, N, x, N, **kw)
    _check(_lib.lib().hqpkkt_debug_symv(device, C.byref(c)), "debug_symv")
    return y, c.chunks


def symv_batch(items, xbase=None, ybase=None, grid_tiles=0, grid_fins=0, device=0):
    """Several products of :func:`symv` in one launch pair (hqpkkt_debug_symv_batch).  items: dicts of symv's arguments (V,
    N, x and the keywords) plus xoff / yoff; xbase: every item reads xbase[xoff: xoff + N] instead of its x; ybase: every
    item writes ybase[yoff: yoff + N] (ybase comes back whole).  grid_tiles / grid_fins: workgroups of the two launches,
    0: one per tile / finishing block.  Returns (list of the items' y - views of ybase where given -, tiles of all items)."""
    import numpy as np
    cs = (_lib.GemvCase * len(items))()
    ys, kept = [], []
    if xbase is not None:
        xbase = np.ascontiguousarray(xbase, dtype=np.float64)
    if ybase is not None:
        assert ybase.dtype == np.float64 and ybase.ndim == 1 and ybase.flags.c_contiguous and ybase.flags.writeable
    for i, it in enumerate(items):
        it = dict(it)
        V, N, x = it.pop("V"), it.pop("N"), it.pop("x", None)
        c, y, _y2, k = _gemv_case(V, N, N, x, N, own_x=xbase is None, own_y=ybase is None, **it)
        cs[i] = c
        kept.append(k)
        ys.append(y if ybase is None else ybase[c.yoff: c.yoff + N])
    _check(_lib.lib().hqpkkt_debug_symv_batch(device, len(items), cs, None if xbase is None else xbase.ctypes.data, 0 if xbase is None else xbase.size,
                                              None if ybase is None else ybase.ctypes.data, 0 if ybase is None else ybase.size, grid_tiles, grid_fins),
           "debug_symv_batch")
    return ys, cs[0].chunks


def symv_map(N):
    """(row tile, column tile) of every tile of the triangle form of order N, in the kernel's tile order (host only,
    hqpkkt_debug_symv_map): an int32 array of tiles x 2."""
    import numpy as np
    tiles = _lib.lib().hqpkkt_debug_symv_map(N, None, 0)
    pairs = np.full((tiles, 2), -1, dtype=np.int32)
    got = _lib.lib().hqpkkt_debug_symv_map(N, pairs.ctypes.data_as(C.POINTER(C.c_int)), pairs.size)
    assert got == tiles
    return pairs


GEMM_FORMS = ("frac", "cut", "plain", "ks", "6432", "6464")  # (what the launch rule can answer; the profile form is asked for)


def gemm_form(M, N, K, lower=False, mirror=False, cus=256, grid=512, sk_tiles=1 << 30, ws_elems=1 << 40, ws2_elems=8 << 20,
              sharded=False, first_stream=True, no_ks=False, no_tile_map=False, force_split=False):
    """The launch rule of the STAGED engine's fp64 product (host only): (form or None, tiles, table wanted, tile order wanted, pieces of k)."""
    flags = sharded * 1 | (not first_stream) * 2 | no_ks * 8 | no_tile_map * 16 | force_split * 32
    tiles, table, tmap, nsplit = C.c_longlong(), C.c_int(), C.c_int(), C.c_int()
    kind = _lib.lib().hqpkkt_debug_gemm_form(M, N, K, int(lower), int(mirror), cus, grid, sk_tiles, ws_elems, ws2_elems, flags,
                                             C.byref(tiles), C.byref(table), C.byref(tmap), C.byref(nsplit))
    return (GEMM_FORMS[kind] if kind >= 0 else None), tiles.value, bool(table.value), bool(tmap.value), nsplit.value


SK_LISTS = {-1: None, 0: "unequal", 1: "equal", 2: "frac", 3: "profile"}


def gemm_caps(cus=256, grid=512, sk_tiles=1 << 30, cnt_elems=None, ws_elems=1 << 40, ws2_elems=8 << 20, variant=2, unequal=True,
              sharded=False, no_ks=False, no_tile_map=False, force_split=False):
    """What the holder of a launch offers :func:`gemm_schedule` (hqpkkt_gemm_caps); cnt_elems None: sk_tiles + 4."""
    return _lib.GemmCaps(variant, cus, grid, int(unequal), sharded * 1 | no_ks * 8 | no_tile_map * 16 | force_split * 32,
                         sk_tiles, sk_tiles + 4 if cnt_elems is None else cnt_elems, ws_elems, ws2_elems)


def gemm_launch(M, N, K, K2=0, lower=False, mirror=False, second_stream=False, ntiles=0, a=0x1000, lda=None, b=0x2000, ldb=None,
                a2=0, lda2=0, b2=0, ldb2=0, mu=0, c=0x4000, ldc=None, c0=None, by=0, panel=None):
    """A launch of the fp64 product described by numbers (hqpkkt_gemm_launch): the addresses are never read.  Defaults: aligned
    operands with even leading dimensions; the segment's columns are the last mu of C."""
    import numpy as np
    up8 = lambda x: (x + 7) // 8 * 8
    ldc = up8(N) if ldc is None else ldc
    l = _lib.GemmLaunch(M, N, K, K2, int(lower), int(mirror), int(second_stream), ntiles, a, b, a2, b2, c,
                        up8(M) if lda is None else lda, up8(N) if ldb is None else ldb, lda2, ldb2, ldc, N - mu if c0 is None else c0, mu, by, None)
    if by:
        l._panel = np.ascontiguousarray(panel, dtype=np.int32).reshape(-1)  # (kept alive with the structure)
        l.panel = l._panel.ctypes.data
    return l


def gemm_schedule(caps, launch, other=None):
    """The schedule of one launch of the STAGED engine's fp64 product (host only, hqpkkt_debug_gemm_schedule): (status, dict)
    with status 0, 1 (no form takes the launch) or 2 (the profile form's list does not fit); the dict holds form, tiles,
    nslab, nsplit, variant, list (None: a plain round), stride, pieces, seg, units[grid, stride, 6] or None, order (int32
    array or None: the kernel's own) and, with `other`, same_key: the two launches share a schedule."""
    import numpy as np
    out = _lib.GemmScheduleOut()
    op = None if other is None else C.byref(other)
    st = _lib.lib().hqpkkt_debug_gemm_schedule(C.byref(caps), C.byref(launch), op, C.byref(out), None, 0, None, 0)
    assert st >= 0
    units = order = None
    if st == 0 and (out.stride > 0 or out.order_len > 0):
        units = np.zeros((caps.grid if out.stride > 0 else 0, out.stride, 6), dtype=np.int32)
        order = np.zeros(out.order_len, dtype=np.int32)
        got = _lib.lib().hqpkkt_debug_gemm_schedule(C.byref(caps), C.byref(launch), op, C.byref(out), units.ctypes.data_as(C.POINTER(C.c_int)), units.size,
                                                    order.ctypes.data_as(C.POINTER(C.c_int)), order.size)
        assert got == 0
    d = {k: getattr(out, k) for k in ("nsplit", "variant", "stride", "tiles", "nslab", "pieces")}
    d.update(form=(GEMM_FORMS + ("profile",))[out.form] if out.form >= 0 else None, list=SK_LISTS[out.list], seg=bool(out.seg),
             same_key=bool(out.same_key), units=units if out.stride > 0 else None, order=order if out.order_len > 0 else None)
    return st, d


def selftest_mfma(device=0):
    err = C.c_double()
    _check(_lib.lib().hqpkkt_selftest_mfma(device, C.byref(err)), "selftest_mfma")
    return err.value
