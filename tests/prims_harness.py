"""Primitive-level differential harness (not a test module, not a conftest).

Drives the sfp_* interface of sorting-fhe_amd/csrc/prims.h directly -- both
libsfhe.so and the oracle library export it -- on CHOSEN residues, and states
every primitive once more in Python integers, from the definitions in prims.h
and from neither implementation.  The tests compare
    oracle == exact            (not marked gpu)
    HIP == exact, HIP == oracle (marked gpu)
with integer equality.  Everything here is plain Python / numpy / ctypes.

Tables are built per (primes, logn) once per process (module-scope caches).
"""
import ctypes as C
import random

import numpy as np

MIN_PRIME_BITS = 30  # modarith.h SF_MIN_PRIME_BITS: what the context and sfp_create accept
FP_BOUND = 1 << 42   # prims_hip.hip kFpPrimeBound: rows below it take the FP64 arithmetic

# --------------------------------------------------------------------------
# number theory in Python integers


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_below(bound, m, avoid=()):
    """Largest prime < bound, = 1 mod m, not in avoid."""
    c = (bound - 2) // m * m + 1
    while not is_prime(c) or c in avoid:
        c -= m
    return c


def prime_above(bound, m, avoid=()):
    c = bound // m * m + m + 1
    while not is_prime(c) or c in avoid:
        c += m
    return c


def find_psi(q, n):
    """A primitive 2n-th root of unity mod q: x^((q-1)/2n) for the smallest x >= 2 that gives one."""
    for x in range(2, q):
        psi = pow(x, (q - 1) // (2 * n), q)
        if pow(psi, n, q) == q - 1:
            return psi
    raise ValueError("no primitive 2n-th root")


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2)


_brev_cache = {}


def brev_table(logn):
    if logn not in _brev_cache:
        r = np.zeros(1, dtype=np.int64)
        for b in range(logn):
            r = np.concatenate([2 * r, 2 * r + 1])
        _brev_cache[logn] = r  # r[k] = brev(k)
    return _brev_cache[logn]


def obj(a):
    """numpy array of Python integers (exact arithmetic)."""
    return np.array([int(v) for v in np.asarray(a).ravel()], dtype=object).reshape(np.shape(a))


def u64(a):
    return np.array(a, dtype=object).astype(np.uint64)


class Ring:
    """The exact arithmetic of one (primes, logn): psi powers in Python integers."""

    def __init__(self, primes, logn):
        self.primes = [int(q) for q in primes]
        self.logn = logn
        self.n = 1 << logn
        self.psi = [find_psi(q, self.n) for q in self.primes]
        self._pw = {}

    def pw(self, p, inverse=False):
        """psi^i (or psi^-i), i < 2n, as an object array."""
        key = (p, inverse)
        if key not in self._pw:
            q = self.primes[p]
            w = pow(self.psi[p], -1, q) if inverse else self.psi[p]
            out, v = [1] * (2 * self.n), 1
            for i in range(1, 2 * self.n):
                v = v * w % q
                out[i] = v
            self._pw[key] = np.array(out, dtype=object)
        return self._pw[key]

    # ---- the tables of sfp_tables, restated from their definition -------------
    def tables(self):
        n, br = self.n, brev_table(self.logn)
        np_ = len(self.primes)
        t = {k: np.zeros((np_, n), dtype=np.uint64) for k in ("psi", "psiS", "ipsi", "ipsiS")}
        ninv, ninvS = [], []
        for p, q in enumerate(self.primes):
            f, i = self.pw(p)[:n][br], self.pw(p, True)[:n][br]  # entry k = psi^brev(k)
            t["psi"][p], t["psiS"][p] = u64(f), u64((f << 64) // q)
            t["ipsi"][p], t["ipsiS"][p] = u64(i), u64((i << 64) // q)
            ni = pow(n, -1, q)
            ninv.append(ni)
            ninvS.append((ni << 64) // q)
        t["ninv"], t["ninvS"] = u64(ninv), u64(ninvS)
        return t

    # ---- negacyclic NTT ----------------------------------------------------
    def _dft(self, b, pw, q):
        """Cyclic DFT sum_i b_i w^(ij), natural order; pw = w^0 .. w^(len/2 - 1)."""
        if len(b) == 1:
            return b
        e, o = self._dft(b[0::2], pw[0::2], q), self._dft(b[1::2], pw[0::2], q)
        t = o * pw % q
        return np.concatenate([(e + t) % q, (e - t) % q])

    def ntt(self, a, p):
        """Output k = sum_i a_i psi^((2 brev(k) + 1) i): the twist by psi^i, then a
        DFT with w = psi^2 (decimation in time, exact integers)."""
        q, n = self.primes[p], self.n
        pw = self.pw(p)
        a = obj(a)
        nz = np.flatnonzero(a != 0)
        if len(nz) <= 1:  # a delta v X^i (or zero): the definition in one term, v psi^(e_k i)
            if not len(nz):
                return a.copy()
            i = int(nz[0])
            return a[i] * pw[(2 * brev_table(self.logn) + 1) * i % (2 * n)] % q
        nat = self._dft(a * pw[:n] % q, pw[0:n:2], q)
        return nat[brev_table(self.logn)]

    def intt(self, A, p):
        q, n = self.primes[p], self.n
        ipw = self.pw(p, True)
        A = obj(A)
        nz = np.flatnonzero(A != 0)
        if len(nz) <= 1:  # one term of the definition
            if not len(nz):
                return A.copy()
            e = 2 * brev(int(nz[0]), self.logn) + 1
            return A[nz[0]] * pow(n, -1, q) * ipw[e * np.arange(n, dtype=np.int64) % (2 * n)] % q
        nat = A[brev_table(self.logn)]  # brev is an involution
        return self._dft(nat, ipw[0:n:2], q) * ipw[:n] % q * pow(n, -1, q) % q

    def ntt_at(self, a, p, k):
        """The definition itself at one output index (O(n))."""
        q, n = self.primes[p], self.n
        e = 2 * brev(k, self.logn) + 1
        pw = self.pw(p)
        idx = (e * np.arange(n, dtype=np.int64)) % (2 * n)
        return int(np.sum(obj(a) * pw[idx]) % q)

    def intt_at(self, A, p, i):
        q, n = self.primes[p], self.n
        ipw = self.pw(p, True)
        e = 2 * brev_table(self.logn) + 1
        return int(np.sum(obj(A) * ipw[(e * i) % (2 * n)]) * pow(n, -1, q) % q)

    # ---- a model of the FP64 forward passes (prims_hip.hip, "FP64 butterflies") ----------
    # The forward transform is the decimation-in-time network over psi_rev: stage S has 2^S
    # groups, group i pairs j and j + t (t = n / 2^(S+1)) with W = psi_rev[2^S + i].  The
    # kernels run it as two passes, stages [0, logn - 8) (COL) and the last 8 (ROW); inside a
    # pass a butterfly is lazy, (a, b) -> (a + r, a - r) with r the centred residue of W b
    # (fpMulMod: b W - rint(b W / q) q), and values return to [0, q) only at the pass's end.
    def fwd_split(self):
        return max(self.logn - 8, 0)

    def psi_rev(self, p):
        return self.pw(p)[:self.n][brev_table(self.logn)]

    def fwd_pass_model(self, a, p):
        """[max |v| / q inside pass 1, inside pass 2] of the lazy model on coefficient row a."""
        q, n, tw = self.primes[p], self.n, self.psi_rev(p)
        v, d1 = obj(a) % q, self.fwd_split()
        peak, out = 0, []
        for S in range(self.logn):
            m, t = 1 << S, n >> (S + 1)
            v = v.reshape(m, 2, t)
            r = v[:, 1, :] * tw[m:2 * m].reshape(m, 1) % q
            r = np.where(r > q // 2, r - q, r)
            v = np.stack([v[:, 0, :] + r, v[:, 0, :] - r], axis=1).reshape(n)
            peak = max(peak, int(np.max(np.abs(v))))
            if S == d1 - 1 or S == self.logn - 1:
                out.append(peak / q)
                peak, v = 0, v % q
        return out

    def fwd_aligned(self, p, which):
        """The coefficient row that drives pass `which` (1 or 2) of the model to its largest
        value, derived from the twiddles: at the pass's entry the head of every sub-transform
        is q - 1 and the partner it meets at stage S holds W_S^-1 h (everything else 0), with
        h just below q / 2 -- so every stage adds +h to the head, which ends at q - 1 + d h
        after the pass's d stages (the model's ceiling is (1 + d / 2) q).  For pass 2 the
        row is the exact inverse of pass 1's stages applied to that entry state."""
        q, n, tw, d1 = self.primes[p], self.n, self.psi_rev(p), self.fwd_split()
        h = (q - 1) // 2 - (q >> 8)  # clear of the tie of rint(b W / q)
        z = np.zeros(n, dtype=object)
        if which == 1:
            cols = n >> d1
            z[:cols] = q - 1
            for S in range(d1):
                t = n >> (S + 1)
                z[t:t + cols] = pow(int(tw[1 << S]), -1, q) * h % q
            return z
        blk = n >> d1
        for i in range(1 << d1):
            z[i * blk] = q - 1
            for k in range(self.logn - d1):
                z[i * blk + (blk >> (k + 1))] = pow(int(tw[(1 << (d1 + k)) + (i << k)]), -1, q) * h % q
        inv2 = pow(2, -1, q)
        for S in range(d1 - 1, -1, -1):  # undo stages d1-1 .. 0 exactly
            m, t = 1 << S, n >> (S + 1)
            z = z.reshape(m, 2, t)
            wi = np.array([pow(int(w), -1, q) for w in tw[m:2 * m]], dtype=object).reshape(m, 1)
            a = (z[:, 0, :] + z[:, 1, :]) * inv2 % q
            b = (z[:, 0, :] - z[:, 1, :]) * inv2 % q * wi % q
            z = np.stack([a, b], axis=1).reshape(n)
        return z

    # ---- automorphism ------------------------------------------------------------
    def aut_perm(self, g):
        """sigma_g(a)(X) = a(X^g): output k is a at the point psi^(e_k g), e_k = 2 brev(k) + 1,
        which is input index brev(((e_k g mod 2n) - 1) / 2)."""
        br = brev_table(self.logn)
        e = (2 * br + 1) * g % (2 * self.n)
        return br[(e - 1) // 2]

    def aut_coeff(self, a, g, q):
        """The substitution X -> X^g on coefficients (X^n = -1)."""
        n = self.n
        out = np.zeros(n, dtype=object)
        for i, v in enumerate(a):
            j = i * g % (2 * n)
            out[j % n] = int(v) % q if j < n else (-int(v)) % q
        return out

    def border_indices(self, seed=1):
        n = self.n
        s = {0, n - 1, 255, 256, 1023, 1024, 2047, 2048, n // 2 - 1, n // 2}
        rng = random.Random(seed)
        s |= {rng.randrange(n) for _ in range(3)}
        return sorted(i for i in s if 0 <= i < n)


_rings = {}


def ring(primes, logn):
    key = (tuple(primes), logn)
    if key not in _rings:
        _rings[key] = Ring(primes, logn)
    return _rings[key]


# --------------------------------------------------------------------------
# the prime sets (issue B).  30 bits is the context's lower limit.


def prime_set(logn):
    """Index: 0 just below 2^60 | 1 30 bits | 2 just below 2^42 (FP64) | 3 just above 2^42
    (integer row between FP64 rows) | 4 32 bits | 5 50 bits | 6 below 2^60 | 7 below 2^42
    | 8 below 2^60 (an integer row at the end of every map)."""
    m = 2 << logn
    p0 = prime_below(1 << 60, m)
    p6 = prime_below(p0, m)
    p8 = prime_below(p6, m)
    p2 = prime_below(FP_BOUND, m)
    p7 = prime_below(p2, m)
    return [p0, prime_below(1 << 30, m), p2, prime_above(FP_BOUND, m), prime_above(1 << 31, m),
            prime_below(1 << 50, m), p6, p7, p8]


def fp_prime_set(logn):
    """prime_set reordered so that q_0 is the only row of 2^42 or more among rows 0..4 (the
    layout of a context with scaling moduli below 2^42): 60 | 30 | below 2^42 | 32 | below 2^42
    | 50 | above 2^42 | P: below 2^42, below 2^60."""
    ps = prime_set(logn)
    return [ps[0], ps[1], ps[2], ps[4], ps[7], ps[5], ps[3], prime_below(ps[7], 2 << logn), ps[8]]


class ConstTerm(C.Structure):
    _fields_ = [("ell", C.c_uint32), ("k", C.c_void_p), ("qlinv", C.c_void_p), ("out", C.c_void_p),
                ("out_stride", C.c_size_t), ("cst", C.c_void_p)]


def small_prime_set(logn):
    """The large rings' four rows: 60 bits, 30 bits, either side of 2^42."""
    m = 2 << logn
    return [prime_below(1 << 60, m), prime_below(1 << 30, m), prime_below(FP_BOUND, m), prime_above(FP_BOUND, m)]


def conv_prime_set(logn):
    """0..2: below 2^60 | 3..15: thirteen FP64 sources (one of 31 bits, the rest below 2^42)
    | 16..20 targets: 30 bits, below 2^42, above 2^42, 50 bits, below 2^60."""
    m = 2 << logn
    out = []
    b = 1 << 60
    for _ in range(3):
        b = prime_below(b, m)
        out.append(b)
    out.append(prime_below(1 << 31, m))
    b = FP_BOUND
    for _ in range(13):
        b = prime_below(b, m)
        out.append(b)
    fp_t = out.pop()  # the thirteenth below 2^42 is a target
    out += [prime_below(1 << 30, m), fp_t, prime_above(FP_BOUND, m), prime_below(1 << 50, m), prime_below(out[2], m)]
    assert len(out) == 21 and len(set(out)) == 21
    return out


# --------------------------------------------------------------------------
# ctypes binding of prims.h


class Limbs(C.Structure):
    _fields_ = [("count", C.c_uint32), ("split", C.c_uint32), ("pbase", C.c_uint32), ("base", C.c_uint32),
                ("stride", C.c_uint32)]

    def primes(self):
        st = self.stride or 1
        return [self.base + i * st if i < self.split else self.pbase + (i - self.split) * st
                for i in range(self.count)]


def ident(count):
    return Limbs(count, count, 0, 0, 0)


class Tables(C.Structure):
    _fields_ = [("logn", C.c_uint32), ("nprimes", C.c_uint32), ("primes", C.c_void_p), ("psi_rev", C.c_void_p),
                ("psi_rev_shoup", C.c_void_p), ("ipsi_rev", C.c_void_p), ("ipsi_rev_shoup", C.c_void_p),
                ("n_inv", C.c_void_p), ("n_inv_shoup", C.c_void_p)]


_T = {"p": C.c_void_p, "u": C.c_uint32, "z": C.c_size_t, "q": C.c_uint64, "i": C.c_int, "L": Limbs}
# name: (result, argument codes after the device handle)
_SIGS = {
    "sfp_alloc": ("p", "z"), "sfp_free": (None, "p"), "sfp_h2d": (None, "ppz"), "sfp_d2h": (None, "ppz"),
    "sfp_sync": (None, ""), "sfp_destroy": (None, ""),
    "sfp_ntt": (None, "pLi"), "sfp_ntt_batch": (None, "pzuLi"),
    "sfp_add": (None, "pppL"), "sfp_sub": (None, "pppL"), "sfp_mul": (None, "pppL"), "sfp_neg": (None, "ppL"),
    "sfp_mul_add": (None, "ppppL"), "sfp_mul_const": (None, "pppL"), "sfp_add_const": (None, "pppL"),
    "sfp_tensor": (None, "pppppppL"), "sfp_tie_tensor": ("i", "pppppppL"),
    "sfp_lin_wsum": (None, "pppuL"), "sfp_lin_wsum_multi": (None, "pzzppupuL"),
    "sfp_mac_plain": (None, "pppuL"), "sfp_mac_plain2": (None, "pppppuL"),
    "sfp_mac_plain2_multi": ("i", "pppppuuL"), "sfp_mac_plain2_cols": ("i", "pppppuuuL"),
    "sfp_automorph": (None, "ppuL"),
    "sfp_rescale": (None, "ppupuzz"), "sfp_rescale_ext": (None, "ppuupuzz"),
    "sfp_mul_const_rescale": (None, "pppupuzz"), "sfp_mul_rescale": (None, "pppupuzz"),
    "sfp_rescale_rows": (None, "pppuLpuzzz"),
    "sfp_rescale_add": ("i", "ppupuzzp"), "sfp_mul_const_rescale_add": ("i", "pppupuzzp"),
    "sfp_upload_conv": ("p", "upuppp p".replace(" ", "")), "sfp_free_conv": (None, "p"),
    "sfp_conv_apply": (None, "ppp"), "sfp_conv_apply_centered": (None, "pppu"),
    "sfp_ks_inner": (None, "pppzpuuuu"), "sfp_ks_inner_acc": (None, "pppzpuuuu"),
    "sfp_ks_inner_aut": (None, "pppzpuuuuu"), "sfp_ks_inner_mul": (None, "pppzpuuuupi"),
    "sfp_ks_inner_mul_aut": (None, "pppzpuuuupiu"), "sfp_ks_inner_fold": (None, "pppzpuuuuppq"),
    "sfp_modup": (None, "ppuuuupp"),
    "sfp_modup_inner": ("i", "pppuuuuppppqiupp"), "sfp_modup_inner_phase": ("i", "pppuuuuppppqiuppi"),
    "sfp_moddown2": (None, "pppzuuuppiipi"),
    "sfp_moddown_rescale": (None, "pppppzuuupppppi"), "sfp_moddown_rescale_add": ("i", "pppppzuuupppppippip"),
    "sfp_mult_relin_rescale": ("i", "ppppppuuuuppppppppp"),
    "sfp_mult_relin_rescale_add": ("i", "ppppppuuuupppppppppppip"),
    "sfp_const_terms_rescale": ("i", "pzupu"),
    "sfp_sample_uniform": (None, "pLq"), "sfp_load_i64": (None, "ppL"), "sfp_sample_small": ("i", "pzuppL"),
    "sfp_modup_prepare": (None, "puuu"),
    # merged launches: batches, stacked regions, lanes, events, graphs
    "sfp_batch_begin": ("i", "u"), "sfp_batch_lane": (None, "u"), "sfp_batch_end": (None, ""),
    "sfp_stack_begin": (None, ""), "sfp_stack_end": (None, ""), "sfp_stack_stats": (None, "pp"),
    "sfp_lanes": ("i", ""), "sfp_set_lane": (None, "i"), "sfp_get_lane": ("i", ""), "sfp_lane_wait": (None, "ii"),
    "sfp_event_record": ("p", ""), "sfp_event_wait": (None, "p"), "sfp_event_free": (None, "p"),
    "sfp_capture_begin": ("i", ""), "sfp_capture_end": ("p", ""), "sfp_graph_launch": (None, "p"),
    "sfp_graph_destroy": (None, "p"), "sfp_graph_nodes": ("z", "p"),
}
_NO_DEV = {"sfp_graph_nodes"}  # (take no device handle)


def _host(a):
    """A host array argument: a contiguous numpy array's address (the caller keeps it alive)."""
    return a.ctypes.data_as(C.c_void_p)


class Dev:
    """One sfp_dev of one library for one (primes, logn)."""

    def __init__(self, lib, primes, logn, device=0):
        self.lib, self.ring = lib, ring(primes, logn)
        self.n, self.logn, self.primes = 1 << logn, logn, [int(q) for q in primes]
        t = self.ring.tables()
        pr = u64(self.primes)
        self._keep = (t, pr)
        tb = Tables(logn, len(primes), _host(pr), _host(t["psi"]), _host(t["psiS"]), _host(t["ipsi"]),
                    _host(t["ipsiS"]), _host(t["ninv"]), _host(t["ninvS"]))
        create = lib.sfp_create
        create.restype, create.argtypes = C.c_void_p, [C.c_int, C.POINTER(Tables)]
        self.d = create(device, C.byref(tb))
        assert self.d, "sfp_create failed"
        le = lib.sfp_last_error
        le.restype, le.argtypes = C.c_char_p, [C.c_void_p]
        self._fn = {}
        self._bufs = []

    def has(self, name):
        return hasattr(self.lib, name)

    def merges(self):
        """Whether this library merges launches at all (the oracle's regions are no-ops)."""
        name = self.lib.sfp_backend_name
        name.restype, name.argtypes = C.c_char_p, []
        return not name().startswith(b"oracle")

    def stats(self):
        """sfp_stack_stats: (launches issued merged, launches issued alone) so far."""
        m, s = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        self.call("sfp_stack_stats", m, s)
        return int(m[0]), int(s[0])

    def stats_delta(self):
        """with D.stats_delta() as got: ...  -- got() is the (merged, single) delta of the block."""
        return _StatsDelta(self)

    def check(self):
        e = self.lib.sfp_last_error(self.d)
        assert e is None, e

    def call(self, name, *args):
        f = self._fn.get(name)
        if f is None:
            f = getattr(self.lib, name)
            res, codes = _SIGS[name]
            f.restype = _T[res] if res else None
            f.argtypes = ([] if name in _NO_DEV else [C.c_void_p]) + [_T[c] for c in codes]
            self._fn[name] = f
        args = [_host(a) if isinstance(a, np.ndarray) else a for a in args]
        r = f(*args) if name in _NO_DEV else f(self.d, *args)
        if name not in ("sfp_free", "sfp_destroy"):
            self.check()
        return r

    # ---- memory ------------------------------------------------------------------
    def alloc(self, words, fill=None):
        p = self.call("sfp_alloc", int(words) * 8)
        assert p and p % 16 == 0
        self._bufs.append(p)
        if fill is not None:
            self.put(p, np.full(int(words), fill, dtype=np.uint64))
        return p

    def put(self, p, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        self.call("sfp_h2d", p, a, a.size * 8)

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        p = self.alloc(a.size)
        self.call("sfp_h2d", p, a, a.size * 8)
        return p

    def down(self, p, shape, offset=0):
        out = np.empty(shape, dtype=np.uint64)
        self.call("sfp_d2h", out, p + 8 * int(offset), out.size * 8)
        return out

    def release(self):
        """Free every buffer of the finished case."""
        self.call("sfp_sync")
        for p in self._bufs:
            self.call("sfp_free", p)
        self._bufs = []

    @staticmethod
    def ptrs(ps):
        return np.array([int(p) for p in ps], dtype=np.uint64)  # a host array of device pointers


class _StatsDelta:
    def __init__(self, D):
        self.D = D

    def __enter__(self):
        self.before = self.D.stats()
        self.after = None
        return lambda: tuple(a - b for a, b in zip(self.after or self.D.stats(), self.before))

    def __exit__(self, *exc):
        self.after = self.D.stats()
        return False


_devs = {}


def dev(lib, tag, primes, logn):
    key = (tag, tuple(primes), logn)
    if key not in _devs:
        _devs[key] = Dev(lib, primes, logn)
    return _devs[key]


# --------------------------------------------------------------------------
# residue patterns (issue C)


def patterns(R, q, seed):
    """name -> row of n residues mod q."""
    n = R.n
    rng = random.Random(seed * 1000003 + q % 1000003)
    out = {}
    for name, v in (("zero", 0), ("one", 1), ("qm1", q - 1), ("half", q >> 1), ("half1", (q >> 1) + 1)):
        out[name] = [v] * n
    for i in R.border_indices():
        row = [0] * n
        row[i] = q - 1
        out["delta%d" % i] = row
    out["alt0"] = [0, q - 1] * (n // 2)
    out["alt1"] = [q - 1, 1] * (n // 2)
    out["uniform"] = [rng.randrange(q) for _ in range(n)]
    return {k: np.array(v, dtype=object) for k, v in out.items()}


def pattern_polys(R, m, seed=7):
    """name -> (object array [count, n], one pattern in every limb of map m)."""
    per = [patterns(R, R.primes[p], seed) for p in m.primes()]
    return {k: np.stack([pp[k] for pp in per]) for k in per[0]}


def exact_rows(R, m, a, fn):
    """fn(row, prime index) per limb of map m."""
    return np.stack([fn(a[i], p) for i, p in enumerate(m.primes())])


def qcol(R, m):
    return np.array([R.primes[p] for p in m.primes()], dtype=object).reshape(-1, 1)


def assert_eq(got, want, what):
    want = u64(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d residues differ; first at %s: got %d, exact %d"
                             % (what, len(bad), got.size, i, got[i], want[i]))


# --------------------------------------------------------------------------
# base-conversion tables and the exact conversions


class ConvRef:
    """Source prime indices S, target prime indices T of a ring's table."""

    def __init__(self, R, S, T, dst_row=None):
        self.R, self.S, self.T = R, list(S), list(T)
        self.s = [R.primes[i] for i in S]
        self.t = [R.primes[i] for i in T]
        self.prod = 1
        for s in self.s:
            self.prod *= s
        self.shat = [self.prod // s for s in self.s]
        self.shat_inv = [pow(h % s, -1, s) for h, s in zip(self.shat, self.s)]
        self.shat_mod = [[h % t for t in self.t] for h in self.shat]
        self.dst_row = list(dst_row) if dst_row is not None else list(range(len(T)))

    def upload(self, D):
        return D.call("sfp_upload_conv", len(self.S), np.array(self.S, dtype=np.uint32), len(self.T),
                      np.array(self.T, dtype=np.uint32), np.array(self.dst_row, dtype=np.uint32),
                      u64(self.shat_inv), u64(self.shat_mod))

    def sources_for(self, y):
        """x_i = y_i shat_i mod s_i: the source rows whose y (prims.h) is the wanted one."""
        return np.stack([y[i] * (self.shat[i] % s) % s for i, s in enumerate(self.s)])

    def y_of(self, x):
        return [obj(x[i]) * self.shat_inv[i] % s for i, s in enumerate(self.s)]

    def plain(self, x):
        """prims.h: out_t = sum_i y_i shat_i mod t, y_i in [0, s_i)."""
        y = self.y_of(x)
        N = sum(yi * h for yi, h in zip(y, self.shat))
        return np.stack([N % t for t in self.t])

    def centred(self, x):
        """The true centred value of x mod prod(S), modulo every target; and per coefficient
        whether it is generic: sum y_i / s_i further than 2^-30 from a half-integer."""
        y = self.y_of(x)
        N = sum(np.where(yi > (s >> 1), yi - s, yi) * h for yi, h, s in zip(y, self.shat, self.s))
        Pm = self.prod
        v = (2 * N + Pm) // (2 * Pm)  # the nearest integer to N / prod
        X = N - v * Pm
        r = N % Pm  # |r / prod - 1/2| < 2^-30  <=>  |2 r - prod| 2^29 < prod
        generic = np.array([abs(2 * int(ri) - Pm) << 29 >= Pm for ri in r])
        return np.stack([X % t for t in self.t]), generic


# --------------------------------------------------------------------------
# splitmix definitions (prims.h: sampling)

_M64 = (1 << 64) - 1


def smix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def exact_uniform(R, m, seed):
    rows = []
    for p in m.primes():
        q = R.primes[p]
        base = smix(seed ^ ((0xD1B54A32D192ED03 * (p + 1)) & _M64))
        rows.append([((smix((base + 2 * x + 1) & _M64) << 64) | smix((base + 2 * x) & _M64)) % q
                     for x in range(R.n)])
    return np.array(rows, dtype=object)


def exact_small(R, m, seed, kind):
    vals = []
    for i in range(R.n):
        r = smix((seed + i) & _M64)
        vals.append(bin(r & 0xFFFFF).count("1") - bin((r >> 20) & 0xFFFFF).count("1") if kind else r % 3 - 1)
    return np.array([[v % R.primes[p] for v in vals] for p in m.primes()], dtype=object)
