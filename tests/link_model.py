"""A NumPy restatement of the link generics of csrc/links.hip, the contract that goes with them, and the sequence generator of
tests/test_gpu_lazy_links.py.

Plain complex128 arithmetic on host images in the oracle layout F[mu, t, z, y, x, b, a] (oracle/oracle.py: _mat, _dag, _ta, _staple_sum, _expm_batch),
one function per generic acting on one (field, slot), the four whole-field calls as loops over them, and an interpreter (Model) that replays a list of
(op, args...) tuples on a dict of fields.  A link is named by a pair ref = (field name, slot), slot = 0..3.

The Model also tracks, per (field, slot), whether the slot is SPECIFIED.  The rule is the documented one (the lazy_links row of the
tunables table; include/lqcd_hip.h, lazy_links): the temporaries of a completed call triple are never written.  So after
    exp(E, t, A) -> mul(W, E, X) -> copy(X, W)                       E and W are unspecified,
    staple(S, U, mu) -> mul(T, U[mu], S) -> add_ta(P[.], f, T)       S and T are unspecified,
and a later write to the whole slot makes it specified again.  The rule is read off the documents, not off links.hip: it is a superset of what the
library leaves unwritten (a triple the recorder does not fuse writes its temporaries, and the comparison merely leaves them out).

Operations (tuples):
    ("copy", dst, src)              ("scaled_copy", dst, s, src)      ("exp", E, t, A)             ("mul", C, A, B)       ("mul_adj", C, A, B)
    ("add_ta", P, f, G)             ("staple", S, Uname, mu, beta)    ("exp_mul", W, t, A, B)      ("add_ta_staple", P, f, Uname, mu, beta)
    ("substitute_U", dstname, srcname)   ("U_update", Uname, Pname, dt)   ("P_update", Uname, Pname, factor, beta)
    ("gauge_force", Gname, Uname, beta)  ("ta_add", Pname, f, Gname)      ("reupload", name, slot, seed)
"""
import numpy as np

from oracle import oracle as _o

FIELDS = ("U", "P", "A", "B")
BETA = 5.7
MAG_CAP = 1e3          # every value the model produces stays below this (the GPU comparison scales by the slot's maximum)


def _m(F, ref):
    """The 3x3 matrices [t, z, y, x, a, b] of one slot (a transposed VIEW of the host image)."""
    return _o._mat(F[ref[0]][ref[1]])


def _put(F, ref, M):
    F[ref[0]][ref[1]] = np.ascontiguousarray(_o._mat(M))


# ---------------------------------------------------------------- the generics, one (field, slot) each
def copy(F, dst, src):
    _put(F, dst, _m(F, src).copy())


def scaled_copy(F, dst, s, src):
    _put(F, dst, s * _m(F, src))


def exp(F, E, t, A):
    _put(F, E, _o._expm_batch(t * _m(F, A)))


def mul(F, C, A, B):
    _put(F, C, _m(F, A) @ _m(F, B))


def mul_adj(F, C, A, B):
    _put(F, C, _o._dag(_m(F, A)) @ _m(F, B))


def add_ta(F, P, f, G):
    _put(F, P, _m(F, P) + f * _o._ta(_m(F, G)))


def staple(F, S, Uname, mu, beta, L):
    _put(F, S, 0.5 * beta * _o._staple_sum(_o._mat(F[Uname]), L, mu))


def exp_mul(F, W, t, A, B):
    _put(F, W, _o._expm_batch(t * _m(F, A)) @ _m(F, B))


def add_ta_staple(F, P, f, Uname, mu, beta, L):
    S = 0.5 * beta * _o._staple_sum(_o._mat(F[Uname]), L, mu)
    _put(F, P, _m(F, P) + f * _o._ta(_m(F, (Uname, mu)) @ S))


# ---------------------------------------------------------------- the whole-field calls: loops over the generics
def substitute_U_(F, dstname, srcname):
    for mu in range(4):
        copy(F, (dstname, mu), (srcname, mu))


def U_update_(F, Uname, Pname, dt):
    for mu in range(4):
        exp_mul(F, (Uname, mu), dt, (Pname, mu), (Uname, mu))


def P_update_(F, Uname, Pname, factor, beta, L):
    """P += factor TA(-(beta/6) U staples) = (-factor/3) TA(U (beta/2) staples), the links unchanged throughout."""
    for mu in range(4):
        add_ta_staple(F, (Pname, mu), -factor / 3.0, Uname, mu, beta, L)


def gauge_force_(F, Gname, Uname, beta, L):
    """G = -(beta/6) U staples, every direction from the links as they were (G is a field of its own)."""
    assert Gname != Uname
    for mu in range(4):
        staple(F, (Gname, mu), Uname, mu, beta, L)
        mul(F, (Gname, mu), (Uname, mu), (Gname, mu))
        scaled_copy(F, (Gname, mu), -1.0 / 3.0, (Gname, mu))


def Traceless_antihermitian_add_(F, Pname, f, Gname):
    for mu in range(4):
        add_ta(F, (Pname, mu), f, (Gname, mu))


# ---------------------------------------------------------------- what an operation reads, writes and exponentiates
def _all(name):
    return [(name, mu) for mu in range(4)]


def reads(op):
    k = op[0]
    if k in ("copy",):
        return [op[2]]
    if k == "scaled_copy":
        return [op[3]]
    if k == "exp":
        return [op[3]]
    if k in ("mul", "mul_adj"):
        return [op[2], op[3]]
    if k == "add_ta":
        return [op[1], op[3]]
    if k == "staple":
        return _all(op[2])
    if k == "exp_mul":
        return [op[3], op[4]]
    if k == "add_ta_staple":
        return [op[1]] + _all(op[3])
    if k == "substitute_U":
        return _all(op[2])
    if k in ("U_update", "P_update"):
        return _all(op[1]) + _all(op[2])
    if k == "gauge_force":
        return _all(op[2])
    if k == "ta_add":
        return _all(op[1]) + _all(op[3])
    if k == "reupload":
        return []
    raise ValueError(op)


def writes(op):
    k = op[0]
    if k in ("copy", "scaled_copy", "exp", "mul", "mul_adj", "add_ta", "staple", "exp_mul", "add_ta_staple"):
        return [op[1]]
    if k in ("substitute_U", "gauge_force", "ta_add"):
        return _all(op[1])
    if k == "U_update":
        return _all(op[1])
    if k == "P_update":
        return _all(op[2])
    if k == "reupload":
        return [(op[1], op[2])]
    raise ValueError(op)


def exponents(op):
    """(ref, t) of every slot the operation exponentiates."""
    if op[0] == "exp":
        return [(op[3], op[2])]
    if op[0] == "exp_mul":
        return [(op[3], op[2])]
    if op[0] == "U_update":
        return [((op[2], mu), op[3]) for mu in range(4)]
    return []


def ta_defect(M):
    """How far the matrices are from traceless anti-Hermitian (absolute, maximum over the sites)."""
    return float(max(np.abs(M + _o._dag(M)).max(), np.abs(np.trace(M, axis1=-2, axis2=-1)).max()))


def max_norm(M):
    """Largest Frobenius norm over the sites."""
    return float(np.sqrt((np.abs(M) ** 2).sum(axis=(-1, -2)).max()))


# ---------------------------------------------------------------- fresh host data, by field
def fresh_slot(name, L, seed):
    """One slot of new host data of the kind the field holds: SU(3) links for U, Gaussian traceless anti-Hermitian momenta for P, general 3x3 else."""
    rng = np.random.default_rng([int(seed), 77])
    shp = (L[3], L[2], L[1], L[0])
    if name == "U":
        M = _o.random_su3(rng, int(np.prod(shp))).reshape(shp + (3, 3))
    elif name == "P":
        M = 1j * np.einsum("...a,aij->...ij", rng.standard_normal(shp + (8,)), _o.GELLMANN / 2)
    else:
        M = rng.standard_normal(shp + (3, 3)) + 1j * rng.standard_normal(shp + (3, 3))
    return np.ascontiguousarray(_o._mat(M))


def initial_fields(L, seed):
    """U: hot start, P: Gaussian momenta, A and B: random general 3x3 (the two temporaries)."""
    F = {"U": _o.hot_gauge(L, seed), "P": _o.gaussian_momenta(L, seed + 1)}
    for k, name in enumerate(("A", "B")):
        F[name] = np.stack([fresh_slot(name, L, 4 * seed + 10 * k + mu) for mu in range(4)])
    return F


# ---------------------------------------------------------------- the interpreter
class UnspecifiedRead(RuntimeError):
    pass


class Model:
    def __init__(self, L, fields):
        self.L = tuple(L)
        self.F = {k: np.array(v, dtype=np.complex128, copy=True) for k, v in fields.items()}
        self.spec = {(k, mu): True for k in self.F for mu in range(4)}
        self.ops = []
        self.exps = []          # (TA defect, |t| * largest norm) of every slot that was exponentiated
        self.peak = 0.0

    def snapshot(self):
        return ({k: v.copy() for k, v in self.F.items()}, dict(self.spec), len(self.ops), len(self.exps), self.peak)

    def restore(self, snap):
        self.F, self.spec, nops, nexp, self.peak = snap[0], snap[1], snap[2], snap[3], snap[4]
        del self.ops[nops:], self.exps[nexp:]

    def apply(self, op):
        F, L, k = self.F, self.L, op[0]
        for r in reads(op):
            if not self.spec[r]:
                raise UnspecifiedRead(f"{op} reads {r}, which the contract leaves unspecified")
        for r, t in exponents(op):
            self.exps.append((ta_defect(_m(F, r)), abs(t) * max_norm(_m(F, r))))
        if k == "copy":
            copy(F, op[1], op[2])
        elif k == "scaled_copy":
            scaled_copy(F, op[1], op[2], op[3])
        elif k == "exp":
            exp(F, op[1], op[2], op[3])
        elif k == "mul":
            mul(F, op[1], op[2], op[3])
        elif k == "mul_adj":
            mul_adj(F, op[1], op[2], op[3])
        elif k == "add_ta":
            assert op[1] != op[3], "add_ta: P and G are the same link field (refused by the entry point)"
            add_ta(F, op[1], op[2], op[3])
        elif k == "staple":
            assert op[1][0] != op[2], "staple: out must not be the link field itself (refused by the entry point)"
            staple(F, op[1], op[2], op[3], op[4], L)
        elif k == "exp_mul":
            exp_mul(F, op[1], op[2], op[3], op[4])
        elif k == "add_ta_staple":
            add_ta_staple(F, op[1], op[2], op[3], op[4], op[5], L)
        elif k == "substitute_U":
            substitute_U_(F, op[1], op[2])
        elif k == "U_update":
            U_update_(F, op[1], op[2], op[3])
        elif k == "P_update":
            P_update_(F, op[1], op[2], op[3], op[4], L)
        elif k == "gauge_force":
            gauge_force_(F, op[1], op[2], op[3], L)
        elif k == "ta_add":
            Traceless_antihermitian_add_(F, op[1], op[2], op[3])
        elif k == "reupload":
            F[op[1]][op[2]] = fresh_slot(op[1], L, op[3])
        else:
            raise ValueError(op)
        for w in writes(op):
            self.spec[w] = True
            self.peak = max(self.peak, float(np.abs(F[w[0]][w[1]]).max()))
        self.ops.append(op)
        self._contract()

    def _contract(self):
        """The temporaries of a call triple that has just completed become unspecified; what its last call wrote stays specified."""
        if len(self.ops) < 3:
            return
        a, b, c = self.ops[-3:]
        temps = None
        if a[0] == "exp" and b[0] == "mul" and c[0] == "copy" and b[2] == a[1] and c[1] == b[3] and c[2] == b[1] and a[1] != b[1]:
            temps = (a[1], b[1])
        if (a[0] == "staple" and b[0] == "mul" and c[0] == "add_ta" and b[2] == (a[2], a[3]) and b[3] == a[1] and c[3] == b[1] and a[1] != b[1]):
            temps = (a[1], b[1])
        if temps:
            for r in temps:
                self.spec[r] = False
            self.spec[c[1]] = True

    def replay(self, ops):
        for op in ops:
            self.apply(op)
        return self

    def specified(self):
        return [r for r in sorted(self.spec) if self.spec[r]]


# ---------------------------------------------------------------- the reference's callers, per direction
def u_triple(mu, t, E=("A", 0), W=("A", 1), U="U", P="P", pslot=None, dst=None):
    """exptU!(E, t, p[mu]); mul!(W, E, U[mu]); substitute_U!(U[mu], W)  (AbstractMD.jl:91-93)"""
    return [("exp", E, t, (P, mu if pslot is None else pslot)), ("mul", W, E, (U, mu)), ("copy", (U, mu) if dst is None else dst, W)]


def p_triple(mu, f, beta=BETA, S=("A", 0), T=("A", 1), U="U", P="P", pslot=None):
    """calc_dSdUmu!(S, ga, mu, U); mul!(T, U[mu], S); Traceless_antihermitian_add!(p[mu], f, T)  (AbstractMD.jl:108-110)"""
    return [("staple", S, U, mu, beta), ("mul", T, (U, mu), S), ("add_ta", (P, mu if pslot is None else pslot), f, T)]


# ---------------------------------------------------------------- the seeded sequence generator
SEQ_L = (4, 4, 6, 2)
MIN_CALLS, MAX_CALLS = 6, 12
_GEN_CAP = 60.0        # the generator drops a call whose result would exceed this: far below MAG_CAP, so that the bound holds with room


class _Gen:
    def __init__(self, seed, L):
        self.rng = np.random.default_rng([int(seed), 0x11CE])
        self.seed, self.L = int(seed), tuple(L)
        self.fields = initial_fields(L, 1000 + 7 * self.seed)
        self.m = Model(L, self.fields)
        self.ops, self.ncalls, self.nfresh = [], 0, 0
        self.t = float(self.rng.choice([0.1, 0.05, -0.08]))
        self.f = float(self.rng.choice([0.02, -0.03]))
        self.order = [int(v) for v in self.rng.permutation(4)]
        self.kind = "U" if self.rng.random() < 0.6 else "P"
        self.nth = 0

    def _fresh(self, ref):
        self.nfresh += 1
        op = ("reupload", ref[0], ref[1], 100000 + 1000 * self.seed + self.nfresh)
        self.m.apply(op)
        self.ops.append(op)

    def emit(self, op):
        """Append one call, after the re-uploads it needs; False (and nothing changed) if the call is not admissible."""
        snap, nops, nfresh = self.m.snapshot(), len(self.ops), self.nfresh
        for r in reads(op):
            if not self.m.spec[r]:
                self._fresh(r)
        ok = True
        for r, t in exponents(op):
            M = _m(self.m.F, r)
            if ta_defect(M) > 1e-12 or abs(t) * max_norm(M) > 1.0:
                if r[0] == "P":
                    self._fresh(r)
                    M = _m(self.m.F, r)
                ok = ok and ta_defect(M) <= 1e-12 and abs(t) * max_norm(M) <= 1.0
        if ok:
            self.m.apply(op)
            ok = self.m.peak <= _GEN_CAP
        if not ok:
            self.m.restore(snap)
            del self.ops[nops:]
            self.nfresh = nfresh
            return False
        self.ops.append(op)
        self.ncalls += 1
        return True

    def room(self):
        return self.target - self.ncalls

    def next_mu(self):
        mu = self.order[self.nth % 4]
        self.nth += 1
        return mu

    def other(self, mu):
        return int(self.rng.choice([s for s in range(4) if s != mu]))

    def temps(self):
        pool = [(n, s) for n in ("A", "B") for s in range(4)]
        i, j = self.rng.choice(len(pool), 2, replace=False)
        return pool[int(i)], pool[int(j)]

    def whole(self, which=None):
        which = which or ("U_update" if self.rng.random() < 0.5 else "P_update")
        return ("U_update", "U", "P", self.t) if which == "U_update" else ("P_update", "U", "P", -3.0 * self.f, BETA)

    def triple(self, kind, mutate):
        mu = self.next_mu()
        E, W = ("A", 0), ("A", 1)
        kw, inter = {}, None
        t, f = self.t, self.f
        if mutate:
            how = str(self.rng.choice(["tmpP", "tmpP2", "tmpU", "dst", "pslot", "pslot", "temps", "inter", "step"]))
            if how == "tmpP":
                E = ("P", self.other(mu))
            elif how == "tmpP2":
                W = ("P", self.other(mu))
            elif how == "tmpU":
                W = ("U", self.other(mu))
            elif how == "dst" and kind == "U":
                kw["dst"] = ("U", self.other(mu))
            elif how in ("pslot", "dst"):
                kw["pslot"] = self.other(mu)
            elif how == "temps":
                E, W = self.temps()
            elif how == "inter":
                inter = int(self.rng.integers(1, 3))
            else:
                t, f = 0.5 * t, 0.5 * f
        if kind == "U" and E == ("P", kw.get("pslot", mu)):
            E = ("A", 0)
        calls = u_triple(mu, t, E, W, **kw) if kind == "U" else p_triple(mu, f, BETA, E, W, **kw)
        if inter is not None:
            calls.insert(inter, self.whole())
        if len(calls) > self.room():
            return
        for op in calls:
            if not self.emit(op):
                return

    def loose(self):
        spec = self.m.specified()
        pool = [(n, s) for n in FIELDS for s in range(4)]
        pick = lambda refs: refs[int(self.rng.integers(len(refs)))]
        dst = pick([r for r in pool if r[0] in ("A", "B")]) if self.rng.random() < 0.8 else pick(pool)
        k = str(self.rng.choice(["copy", "scaled_copy", "mul", "mul_adj", "add_ta"]))
        if k == "copy":
            op = ("copy", dst, pick(spec))
        elif k == "scaled_copy":
            op = ("scaled_copy", dst, float(self.rng.choice([-1.0, 0.5])), pick(spec))
        elif k == "add_ta":
            dst = ("P", int(self.rng.integers(4)))
            op = ("add_ta", dst, self.f, pick([r for r in spec if r != dst]))
        else:
            op = (k, dst, pick(spec), pick(spec))
        self.emit(op)

    def run(self):
        rng = self.rng
        self.target = int(rng.integers(MIN_CALLS, MAX_CALLS + 1))
        start = rng.random()
        if start < 0.25:                                   # a momentum update and the link update behind it wait together
            self.emit(self.whole("P_update"))
            self.emit(self.whole("U_update"))
        elif start < 0.35:
            self.emit(self.whole())
        else:                                              # the callers' own pattern first: up to four clean triples of one update
            for _ in range(int(rng.integers(0, 5))):
                if self.room() >= 3:
                    self.triple(self.kind, False)
        guard = 0
        while self.ncalls < self.target and guard < 200:
            guard += 1
            r = rng.random()
            if r < 0.55 and self.room() >= 3:
                kind = self.kind if rng.random() < 0.7 else ("P" if self.kind == "U" else "U")
                self.triple(kind, rng.random() < 0.5)
            elif r < 0.75:
                self.emit(self.whole())
            else:
                self.loose()
        guard = 0
        while self.ncalls < MIN_CALLS and guard < 200:      # a triple that was cut short by an inadmissible call: fill up
            guard += 1
            self.loose()
        return self.fields, self.ops


def generate(seed, L=SEQ_L):
    """(initial host fields, operations) of one seeded sequence of MIN_CALLS..MAX_CALLS generics (re-uploads not counted)."""
    return _Gen(seed, L).run()


def n_calls(ops):
    return sum(1 for op in ops if op[0] != "reupload")
