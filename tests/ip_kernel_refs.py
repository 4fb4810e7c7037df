"""References of the vector kernels of the device-resident loops (hqp_amd/csrc/ipdriver.hip.h), in plain numpy, for
tests/test_gpu_ip_kernels.py; tests/test_ip_kernel_refs_cpu.py runs what needs no device.  Written from the formulas the
kernel headers cite (Mehrotra's predictor-corrector step with Terlaky's sigma and the damped step length; Franke's cold
start, right-hand sides and ratio test), not from the kernels.

What is EXACT and what is BOUNDED.  fp64 division is correctly rounded, the build has no fast-math, and in `-z / dz`,
`z / dz`, `dz * dw / z / w` no multiply-add can be formed (a product followed by a division), so ratios, their minima
and maxima and the indices are float64 numpy's bits.  Everything else is evaluated in longdouble (unit roundoff 2^-64)
from the exact inputs with a RUNNING ERROR BOUND beside it (class Tr): every operation adds u = 2^-53 times the magnitude
of its result to the errors its operands carry (propagated by the usual first-order rules with the second-order term
kept).  A fused multiply-add rounds once where the uncontracted code rounds twice, so the bound covers both.  A branch
is compared only where the reference's own margin to the threshold exceeds that bound (`margins`, asserted before any
launch); where the arithmetic is exact (ints) the bound is zero and a value may sit on its threshold."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
BIG = 1e300
SLACK = 1.0 + 2.0 ** -10  # the longdouble evaluation's own roundings: 2^-64 = 2^-11 u each, a handful of them


class Tr:
    """A longdouble value and a bound of |computed in double - value|."""

    def __init__(self, v, err=0.0):
        self.v, self.err = LD(v), float(err)

    @staticmethod
    def of(a):
        return a if isinstance(a, Tr) else Tr(a)

    def _new(self, v, err):
        if err == 0.0 and LD(float(v)) == v:
            return Tr(v)  # exact operands and a result a double holds: the correctly rounded operation is exact
        return Tr(v, err + U * float(abs(v)))

    def __add__(self, o):
        o = Tr.of(o)
        return self._new(self.v + o.v, self.err + o.err)

    def __sub__(self, o):
        o = Tr.of(o)
        return self._new(self.v - o.v, self.err + o.err)

    def __mul__(self, o):
        o = Tr.of(o)
        return self._new(self.v * o.v, float(abs(self.v)) * o.err + float(abs(o.v)) * self.err + self.err * o.err)

    def __truediv__(self, o):
        o = Tr.of(o)
        den = float(abs(o.v)) - o.err
        assert den > 0.0, "a divisor that may be zero"
        q = self.v / o.v
        return self._new(q, (self.err + float(abs(q)) * o.err) / den)

    def __neg__(self):
        return Tr(-self.v, self.err)

    def margin(self, t):
        """distance of the value from the threshold t beyond the bound (positive: a rounding cannot flip the comparison)"""
        if self.err == 0.0:
            return np.inf  # exact arithmetic: the device's comparison is the reference's, on the threshold too
        return float(abs(self.v - LD(t))) - self.err

    def close(self, got):
        return abs(LD(got) - self.v) <= LD(self.err * SLACK)

    def ratio(self, got):
        e = float(abs(LD(got) - self.v))
        return 0.0 if e == 0.0 else e / max(self.err * SLACK, 1e-300)


def tmax(a, b):
    return Tr(max(a.v, b.v), max(a.err, b.err))  # |max(a', b') - max(a, b)| <= max of the errors


def tmin(a, b):
    return Tr(min(a.v, b.v), max(a.err, b.err))


# ---- operands

def rng_of(*key):
    return np.random.default_rng([int(k) for k in key])


def step_operands(kind, m, seed, block="both", n=0, me=0):
    """z, w > 0 and a step dz, dw.  ints: entries -8 .. 8 with every ratio z / |dz| a power of two (z = k |dz|, k in 1, 2, 4),
    so that the step length and with it every product and partial sum of (z + alpha dz)(w + alpha dw) is exact.
    block: "none" (all steps >= 0), "z", "w" (only that vector has negative steps), "both"."""
    r = rng_of(seed, m, kind == "ints", ("none", "z", "w", "both").index(block))
    if kind == "ints":
        dz, dw = r.integers(-8, 9, m).astype(float), r.integers(-8, 9, m).astype(float)
        z, w = r.integers(1, 9, m).astype(float), r.integers(1, 9, m).astype(float)
    else:
        dz, dw = r.uniform(-1.0, 1.0, m), r.uniform(-1.0, 1.0, m)
        z, w = r.uniform(0.05, 1.0, m), r.uniform(0.05, 1.0, m)
    if block in ("none", "w"):
        dz = np.abs(dz)
    if block in ("none", "z"):
        dw = np.abs(dw)
    if kind == "ints":
        for v, dv in ((z, dz), (w, dw)):
            neg = dv < 0
            k = 2.0 ** r.integers(0, 3, m)
            k = np.minimum(k, 2.0 ** np.floor(np.log2(8.0 / np.maximum(np.abs(dv), 1.0))))
            v[neg] = (np.abs(dv) * k)[neg]
    out = dict(z=z, w=w, dz=dz, dw=dw)
    if kind == "ints":
        out.update(x=r.integers(-8, 9, n).astype(float), dx=r.integers(-8, 9, n).astype(float),
                   y=r.integers(-8, 9, me).astype(float), dy=r.integers(-8, 9, me).astype(float))
    else:
        out.update(x=r.uniform(-1, 1, n), dx=r.uniform(-1, 1, n), y=r.uniform(-1, 1, me), dy=r.uniform(-1, 1, me))
    return out


# ---- exact parts: ratios, minima, indices

def min_ratio(z, dz):
    """(smallest -z_i / dz_i over dz_i < 0, its first index) or (1e300, -1)"""
    neg = dz < 0.0
    if not neg.any():
        return BIG, -1
    q = np.where(neg, -z / np.where(neg, dz, 1.0), np.inf)
    i = int(np.argmin(q))  # (the first of equal minima)
    return (float(q[i]), i) if q[i] < BIG else (float(q[i]), -1)


def blocking(z, w, dz, dw):
    """k_ip_minratio_final's 12 values"""
    B = []
    for v, dv in ((z, dz), (w, dw)):
        q, i = min_ratio(v, dv)
        B += [q, float(i)] + ([0.0] * 4 if i < 0 else [z[i], dz[i], w[i], dw[i]])
    return np.array(B)


def ratio_stats(z, w, dz, dw):
    """k_ip_ratio's two slots: the smallest ratio of both vectors (1e300 if none) and Terlaky's t"""
    a = min(min_ratio(z, dz)[0], min_ratio(w, dw)[0])
    p = dz * dw
    pos = p > 0.0
    t = float((p[pos] / z[pos] / w[pos]).max()) if pos.any() else 0.0
    return a, t


def clip01(a):
    return max(0.0, min(min(1.0, a), 1.0))


# ---- the step's scalars, tracked

def sigma_ref(a, t, zw_sum, m, gamma):
    """S after the predictor statistics: alpha_aff (exact), sigma and sigma mu (tracked).  mu = zw_sum / m: one correctly
    rounded division in the kernel as here."""
    alpha_aff = clip01(a)
    mu = float(np.float64(zw_sum) / np.float64(m))
    g = Tr(gamma)
    if alpha_aff >= 0.1:  # (alpha_aff is exact: the comparison has no rounding to fear)
        sigma = g * (Tr(t) + 1.0 - alpha_aff) / (Tr(1.0) - g)
    else:
        sigma = g / (Tr(1.0) - g)
    return dict(alpha_aff=alpha_aff, sigma=sigma, smm=sigma * mu, safe=not alpha_aff >= 0.1, mu=mu)


def mupl_sum(z, w, dz, dw, alpha):
    """(z + alpha dz)'(w + alpha dw): m terms of 5 operations each -> (m + 5) u sum of (|z| + |alpha dz|)(|w| + |alpha dw|),
    whatever the order of the sum and the contraction (Higham, section 3.1)"""
    a = LD(alpha)
    s = ((z.astype(LD) + a * dz.astype(LD)) * (w.astype(LD) + a * dw.astype(LD))).sum()
    mag = float(((np.abs(z) + abs(alpha) * np.abs(dz)) * (np.abs(w) + abs(alpha) * np.abs(dw))).sum())
    return Tr(s, (len(z) + 5) * U * mag)


def step_rule_ref(B, m, gamma, gammaf, alpha_aff, sum_of):
    """Mehrotra's step rule from the blocking components B: NEED2, DAMP, alpha before damping (exact), which fpd branch and
    the damped alpha (tracked); sum_of(alpha) gives the tracked sum behind mu_pl.  margins: name -> the reference's own
    margin to a threshold minus the error bound there; every one must be positive."""
    zmin, iz, wmin, iw = B[0], int(B[1]), B[6], int(B[7])
    z_iz, dz_iz, w_iz, dw_iz = B[2:6]
    z_iw, dz_iw, w_iw, dw_iw = B[8:12]
    margins = {}
    amin = min(BIG if iz < 0 else zmin, BIG if iw < 0 else wmin)
    alpha_corr = clip01(amin)
    thr = Tr(gamma) * gamma / 2.0 / float(m) / float(m)
    need2 = bool(alpha_aff >= 0.1 and alpha_corr < thr.v)
    if alpha_aff >= 0.1:
        margins["need2"] = thr.margin(alpha_corr)
    if iz < 0 and iw < 0:
        return dict(need2=need2, damp=False, alpha_pre=1.0, alpha=Tr(0.0 if need2 else 1.0), branch=None, margins=margins, sum=None)
    alpha_pre = wmin if iz < 0 else zmin if iw < 0 else min(zmin, wmin)
    s = sum_of(alpha_pre)
    mu_pl = s / float(m)
    a = Tr(alpha_pre)
    branch = 0
    # "z_iw > -alpha dz_iw": one rounding of the product (contracted or not, the sign of z + alpha dz decides)
    if iw >= 0 and alpha_pre == wmin:
        t = a * dz_iw + z_iw
        margins["fpd_w"] = t.margin(0.0)
        if t.v > 0:
            branch = 1
    if branch == 0 and iz >= 0 and alpha_pre == zmin:
        t = a * dw_iz + w_iz
        margins["fpd_z"] = t.margin(0.0)
        if t.v > 0:
            branch = 2
    if branch == 1:
        fpd = (Tr(gammaf) * mu_pl / (Tr(z_iw) + a * dz_iw) - w_iw) / (a * dw_iw)
    elif branch == 2:
        fpd = (Tr(gammaf) * mu_pl / (Tr(w_iz) + a * dw_iz) - z_iz) / (a * dz_iz)
    else:
        fpd = Tr(0.0)
    alpha = tmax(Tr(0.0), tmin(tmax(Tr(1.0) - gammaf, fpd) * a, Tr(1.0)))
    if need2:
        alpha = Tr(0.0)
    return dict(need2=need2, damp=True, alpha_pre=alpha_pre, alpha=alpha, branch=branch, margins=margins, sum=s)


def step_ref(op, m, gamma, gammaf, alpha_aff):
    B = blocking(op["z"], op["w"], op["dz"], op["dw"])
    r = step_rule_ref(B, m, gamma, gammaf, alpha_aff, lambda a: mupl_sum(op["z"], op["w"], op["dz"], op["dw"], a))
    r["Bk"] = B
    return r


def step_rule_f64(B, s, m, gammaf):
    """ints cases: the rule in float64, operation by operation.  With a power of two for alpha and integer components the
    only roundings are gammaf mu_pl, the two divisions and the subtraction between them - no product feeds an addition,
    so the device must give these bits."""
    zmin, iz, wmin, iw = B[0], int(B[1]), B[6], int(B[7])
    if iz < 0 and iw < 0:
        return 1.0, 1.0
    alpha = wmin if iz < 0 else zmin if iw < 0 else min(zmin, wmin)
    f = np.float64
    mu_pl = f(s) / f(m)
    if iw >= 0 and alpha == wmin and B[8] > -alpha * B[9]:
        fpd = (f(gammaf) * mu_pl / f(B[8] + alpha * B[9]) - f(B[10])) / f(alpha * B[11])
    elif iz >= 0 and alpha == zmin and B[4] > -alpha * B[5]:
        fpd = (f(gammaf) * mu_pl / f(B[4] + alpha * B[5]) - f(B[2])) / f(alpha * B[3])
    else:
        fpd = f(0.0)
    return float(alpha), float(max(0.0, min(max(f(1.0) - f(gammaf), fpd) * f(alpha), 1.0)))


# ---- elementwise and sums

def elem_check(got, terms, ops, label):
    """got against the sum of `terms` (arrays; products already formed in longdouble by the caller as (value, magnitude)
    pairs) with (ops + 1) u sum of magnitudes.  Returns err / bound."""
    ref = sum(t[0] for t in terms)
    mag = sum(t[1] for t in terms)
    bound = (ops + 1) * U * mag
    err = np.abs(got.astype(LD) - ref).astype(float)
    assert not np.isnan(got).any(), label
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (label, bad[:8], err[bad[:8]], bound[bad[:8]])
    return float((err / np.maximum(bound, 1e-300)).max()) if got.size else 0.0


def prod(*f):
    """(longdouble product, magnitude) of arrays / scalars"""
    v, mag = LD(1.0), 1.0
    for a in f:
        v = v * (a.astype(LD) if isinstance(a, np.ndarray) else LD(a))
        mag = mag * np.abs(a)
    return v, mag


def axpy_check(got, x, alpha, dx, label, sign=1.0):
    """x + sign alpha dx: 2 operations"""
    return elem_check(got, [prod(x), prod(sign * alpha, dx)], 2, label)


def sum_check(got, terms_v, terms_mag, c, label):
    """a sum of T terms of c operations each, any order: (T + c) u sum |terms|.  Returns err / bound."""
    T = len(terms_mag)
    bound = (T + c) * U * float(np.sum(terms_mag))
    err = float(abs(LD(got) - np.sum(terms_v.astype(LD) if terms_v.dtype != LD else terms_v)))
    assert err <= bound, (label, err, bound)
    return 0.0 if err == 0.0 else err / bound


# ---- the CSR programs of k_ip_rhs / k_fr_cold

ROW_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 40)


def rows_program(kind, n, me, m, seed):
    """A problems.Program whose Q (full, symmetric), A, C and their transposes have rows of the lengths ROW_LENGTHS among
    others.  Q: a diagonal (absent on a few rows), plus dense little blocks that give rows of every length wanted in the
    symmetric expansion; A and C: see rect (n >= 49; me, m: 0 or >= 49)."""
    from hqp_amd import problems
    r = rng_of(seed, n, me, m, kind == "ints")

    def vals(k):
        if kind == "ints":  # (no zero: a stored entry counts as one in the row lengths below)
            return (r.integers(1, 9, k) * r.choice([-1, 1], k)).astype(float)
        return r.uniform(-1.0, 1.0, k)

    def rect(rows):
        """rows 0 .. 8 have exactly the lengths ROW_LENGTHS (columns from 9 on); column j < 9 has ROW_LENGTHS[j] entries, in
        the rows from 9 on; the rows from 9 on have ROW_LENGTHS[i % 9] entries more"""
        ri, ci = [], []
        for i in range(rows):
            L = min(ROW_LENGTHS[i % 9], n - 9)
            ri += [i] * L
            ci += list(9 + (i * 7 + np.arange(L)) % (n - 9))
        for j in range(9):
            for i in range(9, min(9 + ROW_LENGTHS[j], rows)):
                ri.append(i), ci.append(j)
        return problems._csr(ri, ci, vals(len(ri)), rows)

    # Q's upper triangle: row i of the full matrix has ROW_LENGTHS[i % 9] entries where i < 9 * blocks
    ri, ci = [], []
    length = np.zeros(n, dtype=int)
    for i in range(n):
        want = ROW_LENGTHS[i % 9]
        j = i
        while length[i] < want and j < n:
            if j == i or length[j] < ROW_LENGTHS[j % 9]:
                ri.append(i), ci.append(j)
                length[i] += 1
                if j != i:
                    length[j] += 1
            j += 1
    Q = problems._csr(ri, ci, vals(len(ri)), n)
    A, C = rect(me), rect(m)
    return problems.Program(n, me, m, Q, A, C, c=vals(n), b=vals(me), d=vals(m)), length


def dense_of(csr, rows, cols, sym=False):
    p, i, v = csr
    M = np.zeros((rows, cols))
    for r_ in range(rows):
        M[r_, i[p[r_]:p[r_ + 1]]] = v[p[r_]:p[r_ + 1]]
    if sym:
        M = M + M.T - np.diag(np.diag(M))
    return M


def rhs_ref(kind, prog, x, y, z, w):
    """r1 .. r4 and the six slots of k_ip_rhs.  ints: int64, exact.  reals: (value, bound) per entry - a row of T products
    and the few operations around it: (T + 4) u times the magnitudes - and per slot."""
    n, me, m = prog.dims
    Q, A, C = dense_of(prog.Q, n, n, True), dense_of(prog.A, me, n), dense_of(prog.C, m, n)
    T = LD if kind == "reals" else np.int64
    cv = lambda a: a.astype(T)
    Qx = cv(Q) @ cv(x)
    g = Qx + cv(prog.c)
    r1 = g - cv(A).T @ cv(y) - cv(C).T @ cv(z)
    r2 = -(cv(A) @ cv(x) + cv(prog.b))
    r3 = -(cv(C) @ cv(x) + cv(prog.d) - cv(w))
    r4 = -(cv(z) * cv(w))
    ab = np.abs
    m1 = ab(Q) @ ab(x) + ab(prog.c) + ab(A).T @ ab(y) + ab(C).T @ ab(z)
    m2 = ab(A) @ ab(x) + ab(prog.b)
    m3 = ab(C) @ ab(x) + ab(prog.d) + ab(w)
    T1 = (Q != 0).sum(1) + (A != 0).sum(0) + (C != 0).sum(0)
    T2, T3 = (A != 0).sum(1), (C != 0).sum(1)
    res = dict(r1=(r1, (T1 + 4) * U * m1), r2=(r2, (T2 + 4) * U * m2), r3=(r3, (T3 + 4) * U * m3), r4=(r4, 2 * U * ab(z * w)))
    # slots: gap = x'(Qx + c) + y'b + z'd; pcost = x'(Qx / 2 + c); z'w; max |r|; min z; min w
    gap = cv(x) @ g + cv(y) @ cv(prog.b) + cv(z) @ cv(prog.d)
    if kind == "reals":
        pc = cv(x) @ (LD(0.5) * Qx + cv(prog.c))
    else:
        pc2 = cv(x) @ (Qx + 2 * cv(prog.c))  # twice the cost: an integer
        pc = pc2 / 2.0
    zw = cv(z) @ cv(w)
    gq = ab(x) @ (ab(Q) @ ab(x) + ab(prog.c))
    Tq = int((Q != 0).sum(1).max(initial=0)) + 3  # operations of a term of x'(Qx + c): the row's products, + c, times x
    res["gap"] = (gap, (n + me + m + Tq) * U * (gq + ab(y) @ ab(prog.b) + ab(z) @ ab(prog.d)))
    res["pcost"] = (pc, (n + Tq + 1) * U * gq)
    res["zw"] = (zw, (m + 1) * U * float(ab(z) @ ab(w)))
    return res
