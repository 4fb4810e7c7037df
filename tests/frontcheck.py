"""TEST HELPER: every front of a tree factorisation checked entry by entry (pure numpy / scipy, no GPU import).

A "front source" gives ``structure()``, ``read_block(what, node)`` (the blocks of hqpkkt_debug_read, column-major) and
``stats()``.  ``DeviceSource`` wraps a factorised IpMatrix handle; ``ModelSource`` is a front-by-front float64
factorisation with the pivoting of tests/model.py (``model.bk_block``), laid out as the device lays its blocks, with
hooks that inject single defects the way a wrong kernel would (the fronts above see the defect's consequences
consistently, so that only the identity the defect belongs to breaks).

The host side builds the scaled KKT matrix in elimination numbering from prog, z, w and the SOURCE's scale vector (sparse,
np.longdouble values, with the magnitudes of the summed terms beside them), assembles every front from its original
entries and its children's update blocks as read from the source, and checks with u = 2^-53, p pivots, b border rows, nch
children, all references in np.longdouble:

  a  pivot block   |A11[lp][:,lp] - L11 D L11'|  <= (2p+8) u (|A11| + |L11||D||L11'|)       lower triangle, D from dinv
                   k_factor_blk: + 40 u (|L_iJ||D_J||L_JJ'|)|N_J'||L_JJ'| per 16-block J (see check_fronts)
  b  panel solve   |X - A21[:,lp] tril(M)'|      <= (p+nch+6) u |A21||M'|                   k_panel_solve: a product with M
                   |A21[:,lp] - X L11'|          <= (p+nch+6) u (|A21| + |X||D^-1||D||L11'|)  fused small fronts: substitution
  c  L21           |L21 - X D^-1|                <= 3 u |X||D^-1|
  d  update block  |tril(U) - (ch_BB - L21 X')|  <= (2p+nch+8) u (sum|ch_BB| + |L21||X'|)
  e  triangles     the diagonal 16-blocks of M: zeros above the diagonal, ones on it
  sc               the scale vector against the host's formula to 4 ulp

Every bound carries the underflow term of its operations (2^-1074 each).  Where the source no longer holds an update
block (DeviceSource.u_kept), d of that front is checked through its parent: the parent is assembled from the reference
block and the allowance of d is added to its bounds.
The strict upper triangles of U and of the pivot block are never used.  Fronts whose reference products pass BIG_OPS
multiply-adds take b and d through float64 BLAS against TWICE the bound (both sides then carry the same rounding bound);
the report names them.  check_sweeps() compares one unrefined step with the sweeps of DESIGN section 2 in longdouble on
the source's own blocks."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
from scipy.linalg import solve_triangular

import model

U53 = 2.0 ** -53
LD = np.longdouble
BIG_OPS = 20_000_000
IDS = ("a", "b", "c", "d", "e")
FUSED_KINDS = ("small_fronts", "tree_factor")  # k_factor_diag_small<true>: the whole front in one wavefront


# ------------------------------------------------------------------ the host's side: scale vector, matrix, vectors
def _csr_rows(csr, nrows):
    p, i, x = csr
    p = np.asarray(p, dtype=np.int64)
    return np.repeat(np.arange(nrows), np.diff(p)), np.asarray(i, dtype=np.int64)[: p[-1]], np.asarray(x, dtype=float)[: p[-1]]


def host_scale(prog, z, w, mode):
    """the formulas of model.scaled_kkt for the scale vector, sparse, float64 (QP numbering)"""
    n, me, m = prog.dims
    if mode == 0:
        sc = np.ones(n + me + m)
        wz = w / z
        sc[n + me:] = np.minimum(1.0, np.sqrt(1.0 / wz))
        return sc
    d = np.zeros(n)
    r, c, x = _csr_rows(prog.Q, n)
    on = r == c
    np.add.at(d, r[on], x[on])
    r, c, x = _csr_rows(prog.C, m)
    np.add.at(d, c, x * x * (z / w)[r])
    sc = np.ones(n + me)
    sc[:n] = np.minimum(1.0, np.sqrt(-1.0 / -d))
    return sc


class HostMatrix:
    """The scaled matrix in elimination numbering, lower triangle by columns: ``ptr``, ``row``, ``val`` (longdouble) and
    ``mag`` (the magnitudes of the terms an entry is the sum of, scaled); ``csc`` the same as a scipy matrix (float64)."""

    def __init__(self, prog, z, w, sc, mode, elim):
        n, me, m = prog.dims
        dim = n + me + (m if mode == 0 else 0)
        z, w, sc = (np.asarray(v, dtype=LD) for v in (z, w, sc))
        rows, cols, vals = [], [], []
        r, c, x = _csr_rows(prog.Q, n)
        up = c >= r
        rows.append(r[up]), cols.append(c[up]), vals.append(-x[up].astype(LD))
        r, c, x = _csr_rows(prog.A, me)
        rows.append(n + r), cols.append(c), vals.append(x.astype(LD))
        r, c, x = _csr_rows(prog.C, m)
        if mode == 0:
            rows.append(n + me + r), cols.append(c), vals.append(x.astype(LD))
            k = np.arange(m)
            rows.append(n + me + k), cols.append(n + me + k), vals.append(w / z)
        elif m:
            zw = z / w
            cnt = np.bincount(r, minlength=m)
            one = cnt[r] == 1
            rows.append(c[one]), cols.append(c[one]), vals.append(-(x[one].astype(LD) ** 2) * zw[r[one]])
            start = np.concatenate([[0], np.cumsum(cnt)])
            for k in np.nonzero(cnt > 1)[0]:
                ck, xk = c[start[k]:start[k + 1]], x[start[k]:start[k + 1]].astype(LD)
                ia, ib = np.triu_indices(ck.size)
                rows.append(ck[ia]), cols.append(ck[ib]), vals.append(-xk[ia] * xk[ib] * zw[k])
        qi, qj, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        v = v * sc[qi] * sc[qj]
        e = np.asarray(elim, dtype=np.int64)
        ei, ej = e[qi], e[qj]
        lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
        key = lo * dim + hi
        uk, inv = np.unique(key, return_inverse=True)
        val, mag = np.zeros(uk.size, dtype=LD), np.zeros(uk.size, dtype=LD)
        np.add.at(val, inv, v)
        np.add.at(mag, inv, np.abs(v))
        self.dim, self.n = dim, n
        self.col, self.row, self.val, self.mag = uk // dim, uk % dim, val, mag
        self.ptr = np.searchsorted(self.col, np.arange(dim + 1))
        self.csc = sp.csc_matrix((val.astype(float), self.row, self.ptr), shape=(dim, dim))

    def columns(self, c0, c1):
        a, b = self.ptr[c0], self.ptr[c1]
        return self.row[a:b], self.col[a:b], self.val[a:b], self.mag[a:b]


def scaled_rhs(prog, mode, st, sc):
    """(t, |t| by terms) in QP numbering, longdouble: what k_rhs_full / k_rhs_red_t hand to the sweeps."""
    z, w, r1, r2, r3, r4 = (np.asarray(v, dtype=LD) for v in st)
    sc = np.asarray(sc, dtype=LD)
    n, me, m = prog.dims
    if mode == 0:
        t = np.concatenate([r1, r2, (r4 / z + r3) * sc[n + me:]])
        return t, np.concatenate([np.abs(r1), np.abs(r2), (np.abs(r4 / z) + np.abs(r3)) * sc[n + me:]])
    tz, tza = r4 / w + (z / w) * r3, np.abs(r4 / w) + (z / w) * np.abs(r3)
    r, c, x = _csr_rows(prog.C, m)
    s, sa = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    np.add.at(s, c, x * tz[r])
    np.add.at(sa, c, np.abs(x) * tza[r])
    return np.concatenate([(r1 - s) * sc[:n], r2]), np.concatenate([(np.abs(r1) + sa) * sc[:n], np.abs(r2)])


def unpack(prog, mode, st, sc, xq):
    """(dx, dy, dz, dw) from the solution of the scaled system in QP numbering (k_unpack_full + k_dw, k_unpack_dzdw)."""
    z, w, _r1, _r2, r3, r4 = (np.asarray(v, dtype=float) for v in st)
    n, me, m = prog.dims
    xq, sc = np.asarray(xq, dtype=float), np.asarray(sc, dtype=float)
    r, c, x = _csr_rows(prog.C, m)
    dy = xq[n:n + me].copy()
    if mode == 0:
        dx, dz = xq[:n].copy(), xq[n + me:] * sc[n + me:]
        cdx = np.zeros(m)
        np.add.at(cdx, r, x * dx[c])
        return dx, dy, dz, np.where(w < z, (r4 - w * dz) / z, cdx - r3)
    dx = xq[:n] * sc[:n]
    cdx = np.zeros(m)
    np.add.at(cdx, r, x * dx[c])
    tz = r4 / w + (z / w) * r3
    return dx, dy, tz - (z / w) * cdx, cdx - r3


def solution_e(prog, mode, sc, elim, dx, dy, dz):
    """the sweeps' result in elimination numbering back from a step's (dx, dy, dz): the inverse of the unpack kernels"""
    n, me, m = prog.dims
    sc = np.asarray(sc, dtype=LD)
    if mode == 0:
        xq = np.concatenate([np.asarray(dx, dtype=LD), np.asarray(dy, dtype=LD), np.asarray(dz, dtype=LD) / sc[n + me:]])
    else:
        xq = np.concatenate([np.asarray(dx, dtype=LD) / sc[:n], np.asarray(dy, dtype=LD)])
    out = np.zeros(xq.size, dtype=LD)
    out[np.asarray(elim, dtype=np.int64)] = xq
    return out


# ------------------------------------------------------------------ sources
class DeviceSource:
    def __init__(self, M, plan=None):
        self.M, self.plan, self._pingpong = M, plan, None
        self.s = M.structure()

    def structure(self):
        return self.s

    def stats(self):
        return self.M.stats()

    def read_block(self, what, node):
        return self.M.read_block(what, node)

    def u_kept(self, node):
        """False where the update block has been overwritten since: with update blocks that alternate between two
        half-arenas (hqpkkt_opts.upd_pingpong_mb; the arena is then smaller than all blocks together) a level's blocks
        live until the level after the next has written its own"""
        if self._pingpong is None:
            tot = 8 * int((np.asarray(self.s["nborder"], dtype=np.int64) ** 2).sum())
            self._pingpong = self.M.stats()["bytes_updates"] < tot
        return not self._pingpong or int(self.s["level"][node]) >= int(np.max(self.s["level"])) - 1

    def kind(self, node):
        """the launch kind that factors the front, from the plan's record of its level"""
        if self.plan is None:
            return "?"
        if self.plan["tree_factor"]:
            return "tree_factor"
        R = self.plan["levels"][0][int(self.s["level"][node])]
        p, b = int(self.s["npiv"][node]), int(self.s["nborder"][node])
        if R["fs_n"] and p <= 32 and b <= 16:
            return "small_fronts"
        if R["sm_n"] and p <= 32:
            return "small_blocks"
        return "blk%d" % R["blk_inst"]


def _children(s):
    ch = [[] for _ in range(len(s["npiv"]))]
    for k, par in enumerate(s["parent"]):
        if par >= 0:
            ch[int(par)].append(k)
    return ch


def _front_index(s, k):
    P = np.arange(s["piv_start"][k], s["piv_start"][k] + s["npiv"][k], dtype=np.int64)
    B = np.asarray(s["border_idx"][s["border_ptr"][k]:s["border_ptr"][k + 1]], dtype=np.int64)
    return P, B


def _dinv_blocks(ptype, dinv):
    """[(start, size, D^-1 as a list of lists)] of a front's pivots"""
    out, k, p = [], 0, len(ptype)
    while k < p:
        if ptype[k] == 1:
            out.append((k, 2, [[dinv[2 * k], dinv[2 * k + 1]], [dinv[2 * k + 1], dinv[2 * k + 2]]]))
            k += 2
        else:
            out.append((k, 1, [[dinv[2 * k]]]))
            k += 1
    return out


class ModelSource:
    """Float64 front-by-front factorisation (children's update blocks pulled into the parent, model.bk_block on the pivot
    block, X by substitution, L21 = X D^-1, U = children - L21 X') kept in the device's layout.  ``defect``: (name, node,
    ...) - see _inject."""

    def __init__(self, struct, H, tol=1.0, pivot_eps=1e-10, defect=None, fused=False, lost_u=()):
        self.lost_u = set(lost_u)  # update blocks read_block() no longer gives (NaN instead)
        self.s, self.H, self.fused = struct, H, fused  # fused: X by substitution, as the kernel of the small fronts
        self.defect = defect
        s = struct
        nn = len(s["npiv"])
        ch = _children(s)
        kmax = float(np.abs(H.val).max())
        signs = np.ones(H.dim)
        signs[np.asarray(s["elim"], dtype=np.int64)[: H.n]] = -1.0
        self.blk, self.n2, self.npert, self.perturbed = {}, 0, 0, set()
        where = np.full(H.dim, -1, dtype=np.int64)
        dname, dnode = (defect[0], defect[1]) if defect else (None, -1)
        for k in range(nn):
            P, B = _front_index(s, k)
            p, b = P.size, B.size
            F = p + b
            where[P], where[B] = np.arange(p), p + np.arange(b)
            A = np.zeros((F, F))
            r, c, v, _m = H.columns(P[0], P[-1] + 1)
            v = v.astype(float)
            if dname == "entry" and dnode == k:
                j = np.nonzero((where[r] == defect[2]) & (c - P[0] == defect[3]))[0][0]
                v = v.copy()
                v[j] += 64 * np.spacing(v[j])
            A[where[r], c - P[0]] = v
            for ci, cnode in enumerate(ch[k]):
                Bc = _front_index(s, cnode)[1]
                Uc = self.blk[cnode]["U"]
                Uf = np.tril(Uc) + np.tril(Uc, -1).T
                pos = where[Bc]
                Sc = np.zeros((F, F))
                np.add.at(Sc, (pos[:, None], pos[None, :]), Uf)
                if dname == "child_shift" and dnode == k and ci == defect[2]:  # its part of the update block one position off
                    part = Sc[p:, p:].copy()
                    Sc[p:, p:] = 0.0
                    Sc[p + 1:, p + 1:] = part[:-1, :-1]
                A += Sc
            where[P], where[B] = -1, -1
            A = np.tril(A)
            A11 = A[:p, :p] + np.tril(A[:p, :p], -1).T
            L, blocks, lp, n2, npert = model.bk_block(A11, tol * model.ALPHA0, pivot_eps * kmax, signs[P])
            self.n2 += n2
            self.npert += npert
            if npert:
                self.perturbed.add(k)
            dinv, ptype = np.zeros(2 * p), np.zeros(p)
            for (st, sz, Di) in blocks:
                if sz == 1:
                    dinv[2 * st] = Di[0, 0]
                else:
                    dinv[2 * st:2 * st + 4] = Di[0, 0], Di[1, 0], Di[1, 1], Di[1, 0]
                    ptype[st], ptype[st + 1] = 1, 2
            if dname == "dinv_swap" and dnode == k:
                st = int(np.nonzero(ptype == 1)[0][0])
                dinv[2 * st], dinv[2 * st + 2] = dinv[2 * st + 2], dinv[2 * st]
            Minv = np.tril(solve_triangular(L, np.eye(p), lower=True, unit_diagonal=True))
            if fused:
                X = solve_triangular(L, A[p:, :p][:, lp].T, lower=True, unit_diagonal=True).T if b else np.zeros((0, p))
            else:
                X = A[p:, :p][:, lp] @ Minv.T  # (the product k_panel_solve forms, not a substitution)
            if dname == "x_entry" and dnode == k:
                X[defect[2], defect[3]] += 64 * np.spacing(X[defect[2], defect[3]])
            L21 = np.zeros((b, p))
            for (st, sz, Di) in _dinv_blocks(ptype, dinv):
                L21[:, st:st + sz] = X[:, st:st + sz] @ np.asarray(Di)
            Uk = A[p:, p:].copy()
            if b:
                q = p - 1 if (dname == "drop_last_column" and dnode == k) else p
                Uk -= np.tril(L21[:, :q] @ X[:, :q].T)
                if dname == "diag_twice" and dnode == k:
                    i = defect[2]
                    Uk[i, i] -= L21[i] @ X[i]
            Mstep = Minv.copy()  # (step() below goes on with the inverse as it was computed)
            if dname == "m_entry" and dnode == k:
                Minv[defect[2], defect[3]] += defect[4] * np.spacing(Minv[defect[2], defect[3]])
            panel = np.zeros((F, p))
            panel[:p] = np.tril(L, -1)
            panel[p:] = L21
            self.blk[k] = dict(panel=panel, M=np.tril(Minv), X=X, U=np.tril(Uk), dinv=dinv, ptype=ptype, lperm=lp.astype(float), Mstep=Mstep)
        self._sc = None

    def structure(self):
        return self.s

    def stats(self):
        return dict(n_2x2=self.n2, n_perturbed=self.npert)

    def kind(self, node):
        return "small_fronts" if self.fused else "model"

    def u_kept(self, node):
        return node not in self.lost_u

    def read_block(self, what, node):
        B = self.blk[node]
        if what == 7:
            return self._sc
        key = ("panel", "M", "X", "U", "dinv", "ptype", "lperm")[what]
        v = B[key]
        if what == 3 and node in self.lost_u:
            return np.full(v.size, np.nan)
        return v.ravel(order="F").copy() if v.ndim == 2 else v.copy()

    def step(self, t_e):
        """one unrefined solve in float64, the sweeps as products with M like the kernels': the result in elimination
        numbering"""
        s, x = self.s, np.array(t_e, dtype=float)
        nn = len(s["npiv"])
        for k in range(nn):
            P, B = _front_index(s, k)
            bk = self.blk[k]
            p = P.size
            y = bk["Mstep"] @ x[P][bk["lperm"].astype(int)]
            if B.size:
                x[B] -= bk["panel"][p:] @ y
            for (st, sz, Di) in _dinv_blocks(bk["ptype"], bk["dinv"]):
                y[st:st + sz] = np.asarray(Di) @ y[st:st + sz]
            x[P] = y
        for k in range(nn - 1, -1, -1):
            P, B = _front_index(s, k)
            bk = self.blk[k]
            p = P.size
            v = x[P] - (bk["panel"][p:].T @ x[B] if B.size else 0.0)
            out = np.zeros(p)
            out[bk["lperm"].astype(int)] = bk["Mstep"].T @ v
            x[P] = out
        return x


def model_source(prog, z, w, mode, struct, **kw):
    """ModelSource of the system with the host's own scale vector"""
    sc = host_scale(prog, np.asarray(z, dtype=float), np.asarray(w, dtype=float), mode)
    src = ModelSource(struct, HostMatrix(prog, z, w, sc, mode, struct["elim"]), **kw)
    src._sc = sc
    return src


# ------------------------------------------------------------------ the check
class Report:
    def __init__(self, name):
        self.name = name
        self.worst = {i: (0.0, None) for i in IDS + ("sweep", "sc")}
        self.offenders = {i: [] for i in IDS + ("sweep", "sc")}
        self.fronts = 0
        self.float64_fronts = []
        self.derived_u = []
        self.debug = {}
        self.blocks = {}

    def note(self, ident, ratio, where, entries=()):
        if ratio > self.worst[ident][0]:
            self.worst[ident] = (float(ratio), where)
        for e in entries:
            if len(self.offenders[ident]) < 10:
                self.offenders[ident].append((where, e))

    def failed(self):
        return [i for i in self.worst if self.worst[i][0] > 1.0]

    def ratios(self):
        return {i: self.worst[i][0] for i in self.worst}

    def text(self):
        out = ["%s: %d fronts (%d through float64 products against twice the bound: %s; %d update blocks not held any more, d through the parent)" %
               (self.name, self.fronts, len(self.float64_fronts), self.float64_fronts[:8], len(self.derived_u))]
        for i, (r, wh) in self.worst.items():
            out.append("  %-5s largest err/bound %.4g at %s" % (i, r, wh))
            for wh2, e in self.offenders[i]:
                out.append("        over the bound: %s entry %s" % (wh2, e))
        return "\n".join(out)


TINY = 2.0 ** -1074  # the absolute error of an operation whose result is subnormal


def _over(err, bnd, ident, rep, where, factor=1.0, ops=0):
    """largest err / bound of one identity of one front into the report; entries over the bound with their figures.
    ops: the operations behind an entry - each may underflow (fl(x op y) = (x op y)(1 + delta) + eta, |eta| <= 2^-1074;
    the longdouble reference has the wider exponent and does not)"""
    if err.size == 0:
        return
    bnd = np.asarray(bnd, dtype=float) * factor + ops * TINY
    err = np.asarray(err, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bnd, 0.0)
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    worst = float(ratio.max())
    bad = ()
    if worst > 1.0:
        idx = np.argwhere(ratio > 1.0)[:10]
        bad = [(tuple(int(t) for t in ij), "err %.3e bound %.3e" % (err[tuple(ij)], bnd[tuple(ij)])) for ij in idx]
    rep.note(ident, worst, where, bad)


def _mm(A, B, big):
    if big:
        return np.asarray(A, dtype=float) @ np.asarray(B, dtype=float)
    return np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD)


def check_scale(src, prog, z, w, mode, rep):
    sc = np.asarray(src.read_block(7, 0), dtype=float)
    ref = host_scale(prog, np.asarray(z, dtype=float), np.asarray(w, dtype=float), mode)
    err = np.abs(sc - ref)
    _over(err, 4 * np.spacing(ref), "sc", rep, "scale vector")
    return sc


def check_fronts(src, prog, z, w, mode, name="", keep_blocks=True, exact_leaves=False):
    """a to e over every front of the source, and sc; returns the Report (its ``blocks`` feed check_sweeps)."""
    rep = Report(name)
    s = src.structure()
    sc = check_scale(src, prog, z, w, mode, rep)
    H = HostMatrix(prog, z, w, sc, mode, s["elim"])
    rep.H, rep.sc = H, sc
    nn = len(s["npiv"])
    ch = _children(s)
    where = np.full(H.dim, -1, dtype=np.int64)
    rep.exact_leaves = 0
    derived = {}  # update blocks the source no longer holds: node -> (reference block, its distance bound)
    for k in range(nn):
        P, B = _front_index(s, k)
        p, b, nch = P.size, B.size, len(ch[k])
        F = p + b
        wh = "node %d p %d b %d level %d kind %s" % (k, p, b, int(s["level"][k]), src.kind(k))
        big = p * b * (p + b) > BIG_OPS
        if big:
            rep.float64_fronts.append(k)
        fac = 2.0 if big else 1.0
        # ---- the front as the host assembles it: columns P on rows P | B, lower; children_BB beside it
        where[P], where[B] = np.arange(p), p + np.arange(b)
        A, Am = np.zeros((F, p), dtype=LD), np.zeros((F, p))
        r, c, v, m = H.columns(P[0], P[-1] + 1)
        assert (where[r] >= 0).all(), "an entry outside the symbolic front"
        A[where[r], c - P[0]] = v
        Am[where[r], c - P[0]] = m.astype(float)
        CB, CBm = np.zeros((b, b), dtype=LD), np.zeros((b, b))
        S, SB = np.zeros((F, p)), np.zeros((b, b))  # how far the device's own children may be from the derived ones
        for cnode in ch[k]:
            Bc = _front_index(s, cnode)[1]
            bc = Bc.size
            if cnode in derived:
                Uc, Ec = derived.pop(cnode)
            else:
                Uc, Ec = np.tril(src.read_block(3, cnode).reshape(bc, bc).T).astype(LD), None
            pos = where[Bc]
            assert (pos >= 0).all(), "a child's border row outside the parent's front"
            ip, ib = np.nonzero(pos < p)[0], np.nonzero(pos >= p)[0]
            for blk, into, intoB, absolute in ((Uc, A, CB, False), (Uc, Am, CBm, True), (Ec, S, SB, True)):
                if blk is None:
                    continue
                Uf = blk + np.tril(blk, -1).T
                if absolute:
                    Uf = np.abs(Uf).astype(float)
                if ip.size:  # columns among the pivots: rows at or below them (the lower triangle of the front)
                    sub = Uf[:, ip]
                    rr, cc = np.broadcast_to(pos[:, None], sub.shape), np.broadcast_to(pos[ip][None, :], sub.shape)
                    low = rr >= cc
                    np.add.at(into, (rr[low], cc[low]), sub[low])
                if ib.size:
                    q = pos[ib] - p
                    np.add.at(intoB, (q[:, None], q[None, :]), Uf[np.ix_(ib, ib)])
        where[P], where[B] = -1, -1
        # ---- the source's blocks
        panel = src.read_block(0, k).reshape(p, F).T
        Mfull = src.read_block(1, k).reshape(p, p).T
        dinv, ptype = src.read_block(4, k), src.read_block(5, k).astype(int)
        lp = src.read_block(6, k).astype(int)
        L11 = np.tril(panel[:p], -1) + np.eye(p)
        L21 = panel[p:]
        Mt = np.tril(Mfull)
        # ---- e: triangles, and the consistency of lperm / ptype
        e_bad = []
        if sorted(lp.tolist()) != list(range(p)):
            e_bad.append(("lperm", "not a permutation"))
            lp = np.arange(p)
        for kb in range(0, p, 16):
            blk = Mfull[kb:kb + 16, kb:kb + 16]
            if np.triu(blk, 1).any() or not (np.diag(blk) == 1.0).all():
                e_bad.append((kb, "diagonal 16-block of M: entries above the diagonal or a diagonal that is not 1"))
        t = 0
        while t < p:
            if ptype[t] == 1 and t + 1 < p and ptype[t + 1] == 2:
                if L11[t + 1, t] != 0.0 or dinv[2 * t + 3] != dinv[2 * t + 1]:
                    e_bad.append((t, "2x2 pivot: L(k+1,k) or the second copy of i21"))
                t += 2
            elif ptype[t] == 0:
                t += 1
            else:
                e_bad.append((t, "ptype %d out of sequence" % ptype[t]))
                ptype = ptype.copy()
                ptype[t] = 0
                t += 1
        rep.note("e", np.inf if e_bad else 0.0, wh, e_bad)
        blocks = _dinv_blocks(ptype, dinv)
        # ---- a: pivot block
        A11 = np.tril(A[:p]) + np.tril(A[:p], -1).T
        A11m = np.tril(Am[:p]) + np.tril(Am[:p], -1).T
        D = np.zeros((p, p), dtype=LD)
        for (st, sz, Di) in blocks:
            if sz == 1:
                D[st, st] = LD(1) / LD(Di[0][0]) if Di[0][0] != 0 else np.inf
            else:
                i11, i21, i22 = LD(Di[0][0]), LD(Di[1][0]), LD(Di[1][1])
                det = i11 * i22 - i21 * i21
                D[st:st + 2, st:st + 2] = np.array([[i22, -i21], [-i21, i11]], dtype=LD) / det
        Ll = L11.astype(LD)
        R = (Ll @ D) @ Ll.T
        Rm = (np.abs(L11) @ np.abs(D).astype(float)) @ np.abs(L11).T
        err = np.abs(A11[np.ix_(lp, lp)] - R)
        S11 = np.tril(S[:p]) + np.tril(S[:p], -1).T
        bnd = (2 * p + 8) * U53 * (A11m[np.ix_(lp, lp)] + Rm) + S11[np.ix_(lp, lp)]
        if src.kind(k).startswith("blk"):
            # k_factor_blk (factor_blk.hip.h) works on 16 x 16 blocks, and two of its steps are not the column-by-column
            # elimination that |A11| + |L||D||L'| bounds:
            # - the rows BELOW a diagonal block J are not eliminated pivot by pivot: they are multiplied by the inverse N of
            #   the block's unit lower factor, C_iJ = A'_iJ N' on the matrix pipe (A' the rows as the panels before left
            #   them), L = C D^-1.  That product rounds by 16 u |A'_iJ||N'|, N itself (N L_JJ = I + E, |E| <= 16 u
            #   |N||L_JJ|) enters the same way, and back through L_JJ' both reach A' = C L_JJ' as
            #   (2 16 + 8) u |A'_iJ||N'||L_JJ'| - which the terms of the entry do not bound where N L_JJ cancels;
            # - the diagonal block itself is eliminated as a FULL symmetric image (its mirror half is loaded with it) by
            #   plain Gaussian elimination: L_JJ comes from the multipliers of the lower half, the pivot rows that update
            #   everything behind the block from the upper half, and (x di) y and (y di) x round differently.  The two
            #   halves drift apart by the rounding of the block's own terms, and L_JJ D L_JJ' differs from what the
            #   kernel went on with by that drift taken through N and L_JJ once more - the same product, and its
            #   transpose.  (Seen where a pivot of the block had cancelled to 3e-6 of its terms: tests/test_gpu_tree_fronts.py,
            #   test_2x2_pivots_on_general_fronts and banded20000_12_full.)
            # With |A'_iJ| <= |L_iJ||D_J||L_JJ'| and N the diagonal block of the device's own M (a panel that starts inside
            # a block has a trailing part of it), for every row i from the block's first on:
            Ma, La, Da = np.abs(Mt), np.abs(L11), np.abs(D).astype(float)
            for sj in range(0, p, 16):
                J = slice(sj, min(sj + 16, p))
                Z = (2 * 16 + 8) * U53 * (((La[sj:, J] @ Da[J, J]) @ La[J, J].T) @ Ma[J, J].T) @ La[J, J].T
                bnd[sj:, J] += Z
                bnd[J, J] += Z[:J.stop - sj].T
        tri = np.tril_indices(p)
        ea, ba = np.zeros((p, p)), np.ones((p, p))
        ea[tri], ba[tri] = err[tri].astype(float), bnd[tri]
        _over(ea, ba, "a", rep, wh, ops=2 * p + 8)
        if (ea > ba).any() and len(rep.debug) < 4:  # what a reader of the kernel needs to follow the entry
            hi = A11.astype(float)
            rep.debug[k] = dict(A11_hi=hi, A11_lo=(A11 - hi).astype(float), A11m=A11m, L11=L11, dinv=dinv, ptype=ptype, lperm=lp,
                                panel_diag=np.diag(panel[:p]).copy(), err=ea, bound=ba)
        if b:
            # ---- b: panel solve
            A21, A21m, S21 = A[p:][:, lp], Am[p:][:, lp], S[p:][:, lp]
            X = src.read_block(2, k).reshape(p, b).T
            if src.kind(k) in FUSED_KINDS:
                # The one-wavefront kernel of the small fronts forms no product with M: the border rows take part in the
                # pivot steps, x_j <- fma(-l_k, c_jk, x_j) with l_k = x_k D^-1 and c = L D the unscaled column - forward
                # substitution with L11.  Its identity is X L11' = A21[:,lp]: an entry is a_j less at most p - 1 terms,
                # each through <= 3 roundings of l_k and one of the fma, a_j itself the sum of nch + 1 contributions and
                # <= 3 roundings away from the host's entry - the same (p + nch + 6) u, on the magnitudes of THESE terms,
                # |a_j| + sum |x_k| |D^-1| |D| |L11'| (|c| <= |D||L11'|; for a 1x1 pivot |D^-1||D| = 1).
                G = np.zeros((p, p))
                for (st, sz, Di) in blocks:
                    Dm = np.abs(np.asarray(Di, dtype=float)) @ np.abs(D[st:st + sz, st:st + sz]).astype(float)
                    G[st:st + sz] = Dm @ np.abs(L11).T[st:st + sz]
                _over(np.abs(A21 - X.astype(LD) @ Ll.T), (p + nch + 6) * U53 * (A21m + np.abs(X) @ G) + S21, "b", rep, wh, ops=p + nch + 6)
            else:
                Xr = _mm(A21, Mt.T, big)
                _over(np.abs(X - Xr), (p + nch + 6) * U53 * (A21m @ np.abs(Mt).T) + S21 @ np.abs(Mt).T / fac, "b", rep, wh, fac, ops=p + nch + 6)
            # ---- c: L21 = X D^-1
            Lr, Lm = np.zeros((b, p), dtype=LD), np.zeros((b, p))
            for (st, sz, Di) in blocks:
                Lr[:, st:st + sz] = X[:, st:st + sz].astype(LD) @ np.asarray(Di, dtype=LD)
                Lm[:, st:st + sz] = np.abs(X[:, st:st + sz]) @ np.abs(np.asarray(Di, dtype=float))
            _over(np.abs(L21 - Lr), 3 * U53 * Lm, "c", rep, wh, ops=3)
            # ---- d: update block
            Ur = (CB.astype(float) if big else CB) - _mm(L21, X.T, big)
            Ubnd = (2 * p + nch + 8) * U53 * (CBm + np.abs(L21) @ np.abs(X).T) * fac + SB
            if src.u_kept(k):
                Ud = src.read_block(3, k).reshape(b, b).T
                tri = np.tril_indices(b)
                ed, bd = np.zeros((b, b)), np.ones((b, b))
                ed[tri], bd[tri] = np.abs(Ud - Ur)[tri].astype(float), Ubnd[tri]
                _over(ed, bd, "d", rep, wh, ops=2 * p + nch + 8)
            else:
                # the source has overwritten this block (update blocks that alternate between two half-arenas, level by
                # level): the parent is assembled from the reference block, and what d allows the device's block to
                # differ by is added to every bound of the parent that the block enters
                derived[k] = (np.tril(Ur).astype(LD), np.tril(Ubnd))
                rep.derived_u.append(k)
            if exact_leaves and nch == 0:
                # with exact operands the first pivot's column of X is the front's own entries, untouched
                assert np.array_equal(X[:, 0], A21[:, 0].astype(float)), "exact twin, " + wh
                rep.exact_leaves += 1
        if keep_blocks:
            rep.blocks[k] = (L21.copy(), Mt, dinv, ptype, lp)
        rep.fronts += 1
    return rep


def reference_sweeps(s, blocks, t_e, ta_e):
    """forward and backward sweep of DESIGN section 2 in longdouble on the given blocks, and the same with magnitudes
    and additions: (x, mu) in elimination numbering"""
    x, mu = np.array(t_e, dtype=LD), np.array(ta_e, dtype=LD)
    nn = len(s["npiv"])
    for k in range(nn):
        P, B = _front_index(s, k)
        L21, Mt, dinv, ptype, lp = blocks[k]
        Ml, L2 = Mt.astype(LD), L21.astype(LD)
        y, ya = Ml @ x[P][lp], np.abs(Ml) @ mu[P][lp]
        if B.size:
            x[B] -= L2 @ y
            mu[B] += np.abs(L2) @ ya
        yo, yao = y.copy(), ya.copy()
        for (st, sz, Di) in _dinv_blocks(ptype, dinv):
            Dl = np.asarray(Di, dtype=LD)
            yo[st:st + sz], yao[st:st + sz] = Dl @ y[st:st + sz], np.abs(Dl) @ ya[st:st + sz]
        x[P], mu[P] = yo, yao
    for k in range(nn - 1, -1, -1):
        P, B = _front_index(s, k)
        L21, Mt, _dinv, _ptype, lp = blocks[k]
        Ml, L2 = Mt.astype(LD), L21.astype(LD)
        v, va = x[P], mu[P]
        if B.size:
            v, va = v - L2.T @ x[B], va + np.abs(L2).T @ mu[B]
        o, oa = np.zeros(P.size, dtype=LD), np.zeros(P.size, dtype=LD)
        o[lp], oa[lp] = Ml.T @ v, np.abs(Ml).T @ va
        x[P], mu[P] = o, oa
    return x, mu


def sweep_constant(s):
    levels = int(np.max(s["level"])) + 1
    fmax = int(np.max(np.asarray(s["npiv"]) + np.asarray(s["nborder"])))
    return (2 * levels + 2) * (fmax + 4)


def check_sweeps(rep, s, prog, mode, st, x_e, ident="sweep", where="sweeps"):
    """x_e (elimination numbering) of one unrefined step against the reference sweeps on rep.blocks"""
    e = np.asarray(s["elim"], dtype=np.int64)
    t, ta = scaled_rhs(prog, mode, st, rep.sc)
    te, tae = np.zeros(t.size, dtype=LD), np.zeros(t.size, dtype=LD)
    te[e], tae[e] = t, ta
    xr, mu = reference_sweeps(s, rep.blocks, te, tae)
    err = np.abs(np.asarray(x_e, dtype=LD) - xr)
    _over(err.astype(float), sweep_constant(s) * U53 * mu.astype(float), ident, rep, where)
    return xr
