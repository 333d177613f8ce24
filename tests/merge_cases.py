"""The case table of the merged-launch tests (prims_harness.py, prims_cases.py).

prims_hip.hip glues the launches of independent ops into one ("Stacked launches":
issueSets, launchSets, argSel, issueY / YPay, stackMerge, mergeSets, stackFlush), driven
through sfp_batch_begin / _lane / _end and sfp_stack_begin / _end.  Every case here takes
`devs` like the cases of prims_cases.py, issues several ops on their own buffers inside one
region, and asserts on every library
    integer equality with the exact reference on every output row,
    the fill value past every op's rows,
and on a library that merges (the HIP one; the oracle's regions are no-ops and its
sfp_batch_begin returns 0) the (merged, single) delta of sfp_stack_stats.

The expected delta is not written down per case: flush_model below restates stackFlush's
grouping rule, the cases feed it the launches each op records (read off the host functions,
one token per launch), and the model's pair is asserted exactly.

A host synchronisation (a download) flushes the region, so a case allocates and uploads
first, issues every op, ends the region and only then downloads; case_sync_inside_batch is
the exception, on purpose.
"""
import os

import numpy as np

import prims_cases as K
import prims_harness as H
from prims_harness import Limbs, assert_eq, ident, obj, u64

LOGN = K.LOGN
FILL = 0x5EED5EED
PATS = ("uniform", "qm1", "alt1")


def ntt_fp():
    """SFHE_NTT_FP as prims_hip.hip reads it (default on)."""
    v = os.environ.get("SFHE_NTT_FP")
    return v is None or (v.strip().lstrip("+-").isdigit() and int(v) != 0)


# --------------------------------------------------------------------------
# stackFlush's rule, restated
#
# An item is ("L", cls, key, arg) -- a launch of merge class cls (None: never merged) and key,
# arg: what stackMerge compares besides -- ("R", id) an event record, or ("W", id) a wait for
# record id (0: recorded before the region).  Lanes are listed in lane order.  Each round:
# records and satisfied waits are consumed; among the lanes whose next item is a launch, the
# largest set of one class and key (the first such set on a tie, at most 8) is tried as one
# launch, then with its last lane dropped, ... down to two; if none fits, the lane with the
# most items left (the first on a tie) issues its launch alone -- only the largest set is
# tried, so a refused set also keeps a smaller set of another key waiting.  What fits: the
# element-wise class "Y" takes at most four sets (four argument sets fill the kernel-argument
# block); ModDown + rescale conversions (MDRS) must agree bytewise outside their jobs, i.e.
# be of one table and level (arg).

def fits(heads):
    if heads[0][1] == "Y":
        return len(heads) <= 4
    return len({h[3] for h in heads}) == 1


def flush_model(lanes):
    """-> (merged, single, groups): groups lists every issued launch as (cls, key, lanes)."""
    n = len(lanes)
    at, done, groups = [0] * n, set(), []
    left = lambda l: len(lanes[l]) - at[l]
    head = lambda l: lanes[l][at[l]]
    blocked = lambda l: head(l)[0] == "W" and head(l)[1] and head(l)[1] not in done
    while True:
        moved = True
        while moved:
            moved = False
            for l in range(n):
                while left(l) and head(l)[0] != "L" and not blocked(l):
                    if head(l)[0] == "R":
                        done.add(head(l)[1])
                    at[l] += 1
                    moved = True
        cand = [l for l in range(n) if left(l) and head(l)[0] == "L"]
        if not cand:
            assert not any(left(l) for l in range(n)), "a wait without its record"
            break
        best = []
        for i, l in enumerate(cand):
            a = head(l)
            if a[1] is None:
                continue
            grp = [k for k in cand[i:] if head(k)[1:3] == a[1:3]][:8]
            if len(grp) > len(best):
                best = grp
        nb = len(best)
        while nb >= 2 and not fits([head(l) for l in best[:nb]]):
            nb -= 1
        if nb >= 2:
            groups.append(head(best[0])[1:3] + (tuple(best[:nb]),))
            for l in best[:nb]:
                at[l] += 1
            continue
        one = cand[0]
        for l in cand[1:]:
            if left(l) > left(one):
                one = l
        groups.append(head(one)[1:3] + ((one,),))
        at[one] += 1
    merged = sum(1 for g in groups if len(g[2]) > 1)
    return merged, len(groups) - merged, groups


def L(cls, key, arg=None):
    return ("L", cls, key, arg)


def t_ntt(rows, inverse):
    """sfp_ntt / nttRows above one tile: two passes (forward COL then ROW, inverse ROW then
    COL), the 1024-word-tile kernels up to 64 rows; one key per kernel and grid.x."""
    t = "s" if rows <= 64 else "l"
    return [L("NTT", "ir" + t), L("NTT", "ic" + t)] if inverse else [L("NTT", "fc" + t), L("NTT", "fr" + t)]


def expect(D, got, lanes, what):
    """The stats delta of a library that merges is the model's; the oracle's does not move."""
    if not D.merges():
        assert got == (0, 0), (what, got)
        return None
    m, s, groups = flush_model(lanes)
    print("%s: (merged, single) = %s, derived (%d, %d)" % (what, got, m, s))
    assert got == (m, s), "%s: (merged, single) = %s, stackFlush's rule gives (%d, %d)" % (what, got, m, s)
    return groups


# --------------------------------------------------------------------------
# helpers

_pp = {}


def pp(R, m, seed):
    key = (id(R), tuple(m.primes()), seed)
    if key not in _pp:
        _pp[key] = H.pattern_polys(R, m, seed)
    return _pp[key]


def maps4():
    m = K.maps9()
    return [m["ident"], m["stride"], m["split"], ident(1)]


def out_buf(D, rows, n, fill=FILL):
    """rows + 1 rows of the fill value: the last one is the gap no op may touch."""
    return D.alloc((rows + 1) * n, fill=fill)


def check_out(D, p, rows, n, want, what, fill=FILL):
    got = D.down(p, (rows + 1, n))
    assert_eq(got[:rows], want, what)
    assert (got[rows] == fill).all(), what + ": wrote past its rows"


def run_batch(D, count, issue, declared=None):
    """issue[i]() after sfp_batch_lane(i), inside sfp_batch_begin(count) .. sfp_batch_end;
    -> the stats delta."""
    with D.stats_delta() as got:
        on = D.call("sfp_batch_begin", declared or count)
        assert on == (1 if D.merges() else 0), "sfp_batch_begin(%d) returned %d" % (count, on)
        for i, f in enumerate(issue):
            D.call("sfp_batch_lane", i)
            f()
        D.call("sfp_batch_end")
    return got()


# --------------------------------------------------------------------------
# 1. the element-wise family in a batch

EW_PRIMS = ("add", "mul", "mul_add", "tensor", "automorph", "lin_wsum", "ks_inner")
_ew_specs = {}


def ew_spec(R, prim, i):
    """Op i of a batch of `prim`: its limb map is maps4()[i % 4] (9, 4, 5, 1 rows: grid.x and
    row counts differ inside one launch), the first input's pattern rotates uniform / qm1 /
    alt1 and a further input is a uniform row of the op's own seed.
    -> (rows, nout, host inputs, issue(D, outs, ins), wants)."""
    key = (id(R), prim, i)
    if key in _ew_specs:
        return _ew_specs[key]
    n = R.n
    m = maps4()[i % 4]
    q = H.qcol(R, m)
    if prim in ("add", "mul", "mul_add", "tensor", "automorph"):
        a = pp(R, m, 100 + i)[PATS[i % 3]]
        b = pp(R, m, 200 + i)["uniform"]
        c = pp(R, m, 100 + i)[PATS[(i + 1) % 3]]
        ins = [a, b, c]
        if prim == "add":
            spec = (m.count, 1, ins, lambda D, o, x: D.call("sfp_add", o[0], x[0], x[1], m), [(a + b) % q])
        elif prim == "mul":
            spec = (m.count, 1, ins, lambda D, o, x: D.call("sfp_mul", o[0], x[0], x[1], m), [a * b % q])
        elif prim == "mul_add":
            spec = (m.count, 1, ins, lambda D, o, x: D.call("sfp_mul_add", o[0], x[0], x[1], x[2], m),
                    [(a * b + c) % q])
        elif prim == "tensor":  # (a0, a1) = (a, b), (b0, b1) = (c, a)
            spec = (m.count, 3, ins, lambda D, o, x: D.call("sfp_tensor", o[0], o[1], o[2], x[0], x[1], x[2], x[0], m),
                    [a * c % q, (a * a + b * c) % q, b * a % q])
        else:
            g = K.galois_elements(n)[i % 4]
            spec = (m.count, 1, [b], lambda D, o, x: D.call("sfp_automorph", o[0], x[0], g, m), [b[:, R.aut_perm(g)]])
    elif prim == "lin_wsum":
        nin = (1, 5, 80)[i % 3]
        polys, k = K.sum_inputs(R, m, nin, "half" if nin == 80 else "uniform", 300 + i)
        ins = [polys[0]] if nin == 80 else polys
        want = sum(p * k[j].reshape(-1, 1) for j, p in enumerate(polys)) % q

        def issue(D, o, x, nin=nin, k=u64(k)):
            D.call("sfp_lin_wsum", o[0], D.ptrs(x * nin if len(x) == 1 else x), k, nin, m)
        spec = (m.count, 1, ins, issue, [want])
    else:  # ks_inner: ell 5 / 3 of Lq = 7, K = 2, beta 3 / 2
        ell, beta = ((5, 3), (3, 2))[i % 2]
        Kp, Lq = 2, 7
        rows = ell + Kp
        m = Limbs(rows, ell, Lq, 0, 0)
        q = H.qcol(R, m)
        kr = list(range(ell)) + [Lq, Lq + 1]
        km = ident(Lq + Kp)
        ext = [pp(R, m, 20 + 10 * i + j)[PATS[i % 3] if j == 0 else "uniform"] for j in range(beta)]
        kb = [pp(R, km, 30 + j + 5 * (i % 2))["uniform"] for j in range(beta)]
        ka = [pp(R, km, 40 + j + 5 * (i % 2))["uniform"] for j in range(beta)]
        stride = rows * n + n
        ebuf = np.zeros((beta, stride), dtype=np.uint64)
        for j in range(beta):
            ebuf[j, :rows * n] = u64(ext[j]).ravel()
        key_rows = np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(beta)])
        wants = [sum(e * k_[kr] for e, k_ in zip(ext, kk)) % q for kk in (kb, ka)]
        spec = (rows, 2, [ebuf, key_rows],
                lambda D, o, x: D.call("sfp_ks_inner", o[0], o[1], x[0], stride, x[1], beta, ell, Kp, Lq), wants)
    _ew_specs[key] = spec
    return spec


def ew_tokens(prim):
    """One launch per op: k_ew / k_automorph / k_lin_wsum / k_ks_inner through issueY (class
    Y, one key per kernel); k_tensor is issued unclassified and never merges."""
    return [L(None, "tensor")] if prim == "tensor" else [L("Y", prim)]


def case_ew_batch(devs, prims, count, logn=LOGN):
    """`count` ops in one batch, op i of prim prims[i % len(prims)].

    Derivation (flush_model): the heads of one prim form one group; a group of more than four
    element-wise sets is refused and retried smaller, so count 2, 3, 4 is one launch -- (1, 0)
    -- count 5 is 4 + 1 -- (1, 1) -- and count 8 is 4 + 4 -- (2, 0); sfp_tensor never merges:
    (0, count).  add / mul / add / mul: the adds merge, then the muls: (2, 0)."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    specs = [ew_spec(R, prims[i % len(prims)], i) for i in range(count)]
    lanes = [ew_tokens(prims[i % len(prims)]) for i in range(count)]
    for D in Ds:
        bufs = []
        for rows, nout, ins, _, _ in specs:
            bufs.append(([out_buf(D, rows, n) for _ in range(nout)], [D.up(u64(x)) for x in ins]))
        got = run_batch(D, count, [lambda s=s, b=b: s[3](D, b[0], b[1]) for s, b in zip(specs, bufs)])
        for i, ((rows, nout, _, _, wants), (outs, _)) in enumerate(zip(specs, bufs)):
            for o in range(nout):
                check_out(D, outs[o], rows, n, wants[o], "%s batch of %d, op %d out %d" % ("/".join(prims), count, i, o))
        expect(D, got, lanes, "%s x %d" % ("/".join(prims), count))
        D.release()


# --------------------------------------------------------------------------
# 2. sfp_ntt in a batch

NTT_NAMES = ("uniform", "qm1", "alt1", "alt0", "half", "fwd1", "half1", "fwd2")


def case_ntt_batch(devs, shape, count, logn=LOGN):
    """`count` sfp_ntt in one batch, forward and inverse, op i on pattern NTT_NAMES[i].

    shape "equal": every op on ident(9) -- counts 2, 4, 8 fill their ArgSet and take the
        interleaved rows, counts 3, 5, 6, 7 are padded (the padding sets start at the total
        and get no rows) and concatenated;
    shape "unequal": maps of 9, 4, 5, 1 rows in turn: concatenated, the start[] search;
    shape "directions": ops 0 and 2 forward, 1 and 3 inverse (count 4).

    Derivation: a two-pass transform records two launches of class NTT, keyed by kernel and
    grid.x.  Equal directions: every op's first passes are one launch, then the second
    passes: (2, 0) at every count up to 8.  "directions": the heads are forward COL, inverse
    ROW, forward COL, inverse ROW; the first largest group is lanes 0 and 2, which merge
    twice, then lanes 1 and 3 twice: (4, 0), and no group crosses direction (their kernels,
    hence keys, differ)."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    ms = [ident(9) if shape != "unequal" else maps4()[i % 4] for i in range(count)]
    refs = [K.ntt_reference(R, m)[NTT_NAMES[i]] for i, m in enumerate(ms)]
    for D in Ds:
        for rnd in (0, 1):
            dirs = [(rnd + i) % 2 if shape == "directions" else rnd for i in range(count)]
            bufs = []
            for m, (a, _, _) in zip(ms, refs):
                p = out_buf(D, m.count, n)
                D.put(p, u64(a))
                bufs.append(p)
            got = run_batch(D, count, [lambda p=p, m=m, d=d: D.call("sfp_ntt", p, m, d) for p, m, d in zip(bufs, ms, dirs)])
            for i, (p, m, d) in enumerate(zip(bufs, ms, dirs)):
                check_out(D, p, m.count, n, refs[i][1 + d], "ntt batch %s of %d, op %d inverse=%d" % (shape, count, i, d))
            groups = expect(D, got, [t_ntt(m.count, d) for m, d in zip(ms, dirs)], "ntt %s x %d round %d" % (shape, count, rnd))
            if groups and shape == "directions":
                assert [g[2] for g in groups] == [(0, 2), (0, 2), (1, 3), (1, 3)], groups
            D.release()


def case_ntt_batch_tiles(devs, logn=LOGN):
    """One sfp_ntt_batch of 8 x 9 = 72 rows (more than 64: the 2048-word tiles, grid.x = n / 2048)
    next to two 9-row sfp_ntt (1024-word tiles, grid.x = n / 1024), forward and inverse.

    Derivation: kernel and grid.x differ between the tile sizes, so the keys differ: the two
    small transforms are the only group of two and merge pass by pass, then the large one
    issues its two passes alone: (2, 2)."""
    R, Ds = K.setup(devs, logn)
    n, m = R.n, ident(9)
    ref = K.ntt_reference(R, m)
    names = list(ref)
    stride = 9 * n + n
    sel = np.arange(8) % len(names)

    def lay(which):
        buf = np.full((8, stride), FILL, dtype=np.uint64)
        buf[:, :9 * n] = np.stack([u64(ref[names[j]][which]) for j in sel]).reshape(8, -1)
        return buf

    small = [ref["fwd2"], ref["alt0"]]
    for D in Ds:
        for d in (0, 1):
            big = D.up(lay(0))
            ps = []
            for a, _, _ in small:
                p = out_buf(D, 9, n)
                D.put(p, u64(a))
                ps.append(p)
            got = run_batch(D, 3, [lambda: D.call("sfp_ntt_batch", big, stride, 8, m, d),
                                   lambda: D.call("sfp_ntt", ps[0], m, d), lambda: D.call("sfp_ntt", ps[1], m, d)])
            assert np.array_equal(D.down(big, (8, stride)), lay(1 + d)), "ntt_batch of 72 rows inside a batch, inverse=%d" % d
            for j in (0, 1):
                check_out(D, ps[j], 9, n, small[j][1 + d], "9-row ntt next to the 72-row one, op %d inverse=%d" % (j, d))
            groups = expect(D, got, [t_ntt(72, d), t_ntt(9, d), t_ntt(9, d)], "ntt tiles inverse=%d" % d)
            if groups:
                assert [g[2] for g in groups] == [(1, 2), (1, 2), (0,), (0,)], groups
            D.release()


# --------------------------------------------------------------------------
# 3. conversions in a batch

CONV_TABLES = ((1, 0), (2, 1), (12, 0))  # (ns, 60-bit sources): all at most 13 sources, one kernel form
ONE_T, ONE_ROW = [17], [1]
_conv_x = {}


def case_conv_batch(devs, count, logn=LOGN):
    """`count` conversions in one batch.  Op i: table CONV_TABLES[i % 3]; the one target 17 (row 1)
    for even i, targets CONV_T (five, rows CONV_ROWS: two FP64 and three integer rows, a block
    layer each) for odd i, so the first head is shallower in grid.z than a later one; sfp_conv_apply_centered (nt_use 3 of 5, or 1 of 1) where (i // 2) is odd, else
    sfp_conv_apply; generic_y inputs, so the centred result is exact.  From count 3 on the last
    op is centred on near-tie inputs (tie_y, table (12, 0), five targets): exact or exact
    +- prod(S), the same choice on every target.

    Derivation: every conversion records one launch of class CONV keyed by kernel form and
    grid.x, which all share; the jobs (count <= 16) are joined into one table and one launch
    with grid.z the maximum over the heads: (1, 0)."""
    R, Ds = K.setup(devs, logn, H.conv_prime_set(logn))
    n = R.n
    ops = []
    for i in range(count):
        ns, nbig = CONV_TABLES[i % 3]
        one = i % 2 == 0
        tie = count >= 3 and i == count - 1
        if tie:
            ns, nbig, one = 12, 0, False
        cr = H.ConvRef(R, K.conv_sources(ns, nbig), ONE_T if one else K.CONV_T, ONE_ROW if one else K.CONV_ROWS)
        centred = tie or (i // 2) % 2 == 1
        key = (id(R), ns, nbig, one, "tie" if tie else i)
        if key not in _conv_x:
            _conv_x[key] = K.tie_y(R, cr)[2] if tie else K.generic_y(R, cr, 7000 + 10 * i)
        ops.append((cr, centred, (1 if one else 3) if centred else len(cr.T), tie, _conv_x[key]))
    for D in Ds:
        tabs, srcs, dsts = [], [], []
        for cr, _, _, _, x in ops:
            tabs.append(cr.upload(D))
            srcs.append(D.up(u64(x)))
            dsts.append(out_buf(D, 7, n, 0x4444))

        def issue(i):
            cr, centred, nt_use, _, _ = ops[i]
            if centred:
                D.call("sfp_conv_apply_centered", dsts[i], srcs[i], tabs[i], nt_use)
            else:
                D.call("sfp_conv_apply", dsts[i], srcs[i], tabs[i])
        got = run_batch(D, count, [lambda i=i: issue(i) for i in range(count)])
        for i, (cr, centred, nt_use, tie, x) in enumerate(ops):
            out = D.down(dsts[i], (8, n))
            what = "conv batch of %d, op %d" % (count, i)
            written = cr.dst_row[:nt_use]
            for r in range(8):
                if r not in written:
                    assert (out[r] == 0x4444).all(), what + ": wrote row %d" % r
            if not centred:
                want = cr.plain(x)
                for t, r in enumerate(cr.dst_row):
                    assert_eq(out[r], want[t], what + " target %d" % t)
                continue
            wc, generic = cr.centred(x)
            assert tie or generic.all()
            choice = None
            for t in range(nt_use):
                tq = cr.t[t]
                d = (obj(out[cr.dst_row[t]]) - wc[t]) % tq
                pm = cr.prod % tq
                ch = np.where(d == 0, 0, np.where(d == pm, 1, np.where(d == (-pm) % tq, -1, 9)))
                assert not (ch[generic] != 0).any(), what + " target %d: a generic coefficient is not exact" % t
                assert not (ch == 9).any(), what + ": neither exact nor exact +- prod(S)"
                assert choice is None or np.array_equal(choice, ch), what + ": targets disagree on the overflow"
                choice = ch
        expect(D, got, [[L("CONV", "c")] for _ in ops], "conv x %d" % count)
        D.call("sfp_sync")
        for c in tabs:
            D.call("sfp_free_conv", c)
        D.release()


# --------------------------------------------------------------------------
# 4 / 5. key-switch chains in a batch

_chain = {}


def chain_tables(R, ell):
    key = ("tab", id(R), ell)
    if key not in _chain:
        _chain[key] = K.ks_convs(R, ell, K.KS["K"], K.KS["Lq"], K.KS["alpha"])
    return _chain[key]


def chain_key(R):
    """The switching key's three digits (b rows then a rows of Lq + K limbs): shared by every op;
    an op of fewer digits reads a prefix."""
    key = ("key", id(R))
    if key not in _chain:
        km = ident(K.KS["Lq"] + K.KS["K"])
        _chain[key] = ([pp(R, km, 30 + j)["uniform"] for j in range(3)], [pp(R, km, 40 + j)["uniform"] for j in range(3)])
    return _chain[key]


def chain_inputs(R, ell, i):
    """Op i's own rows: a uniform input of its own seed, d0 / d1 rotating the patterns."""
    return (pp(R, ident(ell), 500 + i)["uniform"], pp(R, ident(ell), 520 + i)[PATS[i % 3]],
            pp(R, ident(ell), 540 + i)[PATS[(i + 1) % 3]])


def chain_consts(R, ell):
    Kp, Lq = K.KS["K"], K.KS["Lq"]
    _, down = chain_tables(R, ell)
    l, P = ell - 1, down.prod
    return (u64([pow(P, -1, R.primes[i]) for i in range(ell)]), u64([P % R.primes[i] for i in range(ell)]),
            u64([pow(R.primes[l], -1, R.primes[i]) for i in range(l)]), P % R.primes[l])


def chain_exact(pset, ell, i, logn=LOGN):
    """The exact chain of op i at level ell (cached): ModUp's digits; the outputs of
    sfp_moddown_rescale (even i; after sfp_ks_inner_fold) or of sfp_ks_inner + sfp_moddown2
    (odd i); sfp_mult_relin_rescale's outputs for the operands (d0, in) x (d1, in)."""
    key = ("exact", pset, ell, i, logn)
    if key in _chain:
        return _chain[key]
    R = H.ring(K.ks_primes(pset, logn), logn)
    Kp, Lq, alpha = K.KS["K"], K.KS["Lq"], K.KS["alpha"]
    rows, beta = ell + Kp, (ell + alpha - 1) // alpha
    up, down = chain_tables(R, ell)
    inp, d0, d1 = chain_inputs(R, ell, i)
    kb, ka = chain_key(R)
    q, ql = H.qcol(R, Limbs(rows, ell, Lq, 0, 0)), H.qcol(R, ident(ell))
    kr = list(range(ell)) + [Lq + k for k in range(Kp)]
    fold_k = down.prod % R.primes[ell - 1]
    ext = K.exact_modup(R, inp, up, ell, Kp)
    s = [sum(e * k_[kr] for e, k_ in zip(ext, kk[:beta])) % q for kk in (kb, ka)]
    if i % 2 == 0:
        out = [K.exact_md_rescale(R, s[p], (d0, d1)[p], down, ell, Kp, Lq, fold_k) for p in range(2)]
    else:
        out = [K.exact_moddown(R, s[p], down, ell, Kp, Lq)[0] for p in range(2)]
    t0, t1, t2 = d0 * d1 % ql, (d0 * inp + inp * d1) % ql, inp * inp % ql
    ext2 = K.exact_modup(R, t2, up, ell, Kp)
    s2 = [sum(e * k_[kr] for e, k_ in zip(ext2, kk[:beta])) % q for kk in (kb, ka)]
    mrr = [K.exact_md_rescale(R, s2[p], (t0, t1)[p], down, ell, Kp, Lq, fold_k) for p in range(2)]
    _chain[key] = (ext, out, mrr)
    return _chain[key]


def chain_plan(R, ell):
    """Whether sfp_modup fuses the conversion into its forward COL pass (modupPlan): FP64 on and
    q_0 the only source row of 2^42 or more."""
    return ntt_fp() and all(R.primes[r] < H.FP_BOUND for r in range(1, ell))


def chain_tokens(R, ell, i, fused):
    """The launches op i records, from the host functions:
    sfp_modup: the input's inverse NTT (ROW, COL); with a plan the conversion rides in the
        forward COL pass (its own kernel: the CONV form at 2^12, k_modup_col -- two targets a
        block at these sizes -- at 2^16), else one conversion launch and the plain COL pass;
        the forward ROW pass;
    sfp_ks_inner(_fold): one k_ks_inner (class Y);
    sfp_moddown_rescale: inverse NTT of the dropped row and the P rows, the conversion (class
        MDRS, keyed by kernel, grid.x and grid.z: the ModDown table of both prime sets has a
        60-bit source, so every level runs k_mdrsi with grid.z = ceil(l / 32) = 1: one key; merged only with heads of its own table and level,
        the bytewise compare), forward NTT with the epilogue;
    sfp_moddown2: inverse NTT of the P rows, one conversion launch (two jobs), forward NTT;
    sfp_mult_relin_rescale (`fused`): inverse NTT, conversion as in sfp_modup, the forward COL
        pass, k_ntt_ks (class KS), the inverse COL pass of the accumulators' tail (their ROW
        pass ran inside k_ntt_ks), the MDRS conversion, forward NTT.
    Every launch here has at most 64 rows: the 1024-word-tile kernels."""
    plan = chain_plan(R, ell)
    col = ("mc" if R.logn == 16 else "fcC") if plan else "fc"
    conv = [] if plan else [L("CONV", "c")]
    mdrs = [L("MDRS", "m", ell - 1)]
    t = t_ntt(1, 1) + conv + [L("NTT", col + "s"), L("NTT", "frs")] + [L("Y", "ks_inner")]
    if i % 2 == 0:
        t += t_ntt(1, 1) + mdrs + t_ntt(1, 0)
    else:
        t += [L("Y", "ks_inner")] + t_ntt(1, 1) + [L("CONV", "c")] + t_ntt(1, 0)
    if fused:
        t += t_ntt(1, 1) + conv + [L("NTT", col + "s"), L("KS", "s"), L("NTT", "ics")] + mdrs + t_ntt(1, 0)
    return t


class ChainOp:
    """One op's device buffers (its own outputs and scratch) and its call sequence."""

    def __init__(self, D, R, ell, i, tabs):
        Kp, Lq, alpha = K.KS["K"], K.KS["Lq"], K.KS["alpha"]
        n = R.n
        self.D, self.R, self.ell, self.i, self.n = D, R, ell, i, n
        self.rows, self.beta = ell + Kp, (ell + alpha - 1) // alpha
        inp, d0, d1 = chain_inputs(R, ell, i)
        self.IN, self.D0, self.D1 = D.up(u64(inp)), D.up(u64(d0)), D.up(u64(d1))
        self.E, self.E2 = D.alloc(self.beta * self.rows * n, fill=FILL), D.alloc(self.beta * self.rows * n)
        self.scr, self.acc = D.alloc(2 * ell * n), D.alloc(2 * self.rows * n)
        self.nout = ell - 1 if i % 2 == 0 else ell
        self.o = [out_buf(D, self.nout, n) for _ in range(2)]
        self.m = [out_buf(D, ell - 1, n) for _ in range(2)]
        self.cv_keep, self.cv, self.cP, self.KEY = tabs
        self.fused = None

    def issue(self):
        D, n, ell, rows, beta = self.D, self.n, self.ell, self.rows, self.beta
        Kp, Lq, alpha = K.KS["K"], K.KS["Lq"], K.KS["alpha"]
        pinv, pmod, qlinv, fold_k = chain_consts(self.R, ell)
        acc1 = self.acc + rows * n * 8
        D.call("sfp_modup", self.E, self.IN, ell, Kp, Lq, alpha, self.cv, self.scr)
        D.call("sfp_ks_inner_fold", self.acc, acc1, self.E, rows * n, self.KEY, beta, ell, Kp, Lq, self.D0, self.D1, fold_k)
        if self.i % 2 == 0:
            D.call("sfp_moddown_rescale", self.o[0], self.o[1], self.D0, self.D1, self.acc, rows * n, ell, Kp, Lq, self.cP,
                   pinv, pmod, qlinv, self.scr, 0)
        else:
            D.call("sfp_ks_inner", self.acc, acc1, self.E, rows * n, self.KEY, beta, ell, Kp, Lq)
            D.call("sfp_moddown2", self.o[0], self.o[1], self.acc, rows * n, ell, Kp, Lq, self.cP, pinv, 0, 0, self.scr, 0)
        r = D.call("sfp_mult_relin_rescale", self.m[0], self.m[1], self.D0, self.IN, self.D1, self.IN, ell, Kp, Lq, alpha,
                   self.cv, self.KEY, self.cP, pinv, pmod, qlinv, self.acc, self.E2, self.scr)
        assert r in (0, -1)
        self.fused = r == 0

    def mrr_unfused(self):
        """sfp_mult_relin_rescale's definition from the unfused prims (a library without the fused
        form): the tensor, ModUp of d2, the inner product with d0 / d1 folded, ModDown + rescale."""
        D, n, ell, rows, beta = self.D, self.n, self.ell, self.rows, self.beta
        Kp, Lq, alpha = K.KS["K"], K.KS["Lq"], K.KS["alpha"]
        pinv, pmod, qlinv, fold_k = chain_consts(self.R, ell)
        acc1 = self.acc + rows * n * 8
        T = [D.alloc(ell * n) for _ in range(3)]
        D.call("sfp_tensor", T[0], T[1], T[2], self.D0, self.IN, self.D1, self.IN, ident(ell))
        D.call("sfp_modup", self.E2, T[2], ell, Kp, Lq, alpha, self.cv, self.scr)
        D.call("sfp_ks_inner_fold", self.acc, acc1, self.E2, rows * n, self.KEY, beta, ell, Kp, Lq, T[0], T[1], fold_k)
        D.call("sfp_moddown_rescale", self.m[0], self.m[1], T[0], T[1], self.acc, rows * n, ell, Kp, Lq, self.cP,
               pinv, pmod, qlinv, self.scr, 0)

    def refill(self):
        """After the warm-up run: the outputs back to their fill."""
        D, n = self.D, self.n
        D.put(self.E, np.full(self.beta * self.rows * n, FILL, dtype=np.uint64))
        for p in self.o:
            D.put(p, np.full((self.nout + 1) * n, FILL, dtype=np.uint64))
        for p in self.m:
            D.put(p, np.full(self.ell * n, FILL, dtype=np.uint64))


def chain_devices(D, R, ells):
    """Per level: the uploaded ModUp tables (host pointer array kept alive), the ModDown table; the
    key.  sfp_modup_prepare builds the fused ModUp's per-level tables now: built on first use
    they would be uploaded -- a host synchronisation -- in the middle of the region."""
    kb, ka = chain_key(R)
    KEY = D.up(np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(3)]))
    tabs, handles = {}, []
    for ell in sorted(set(ells)):
        up, down = chain_tables(R, ell)
        cj = [c.upload(D) for c in up]
        assert all(cj)
        cP = down.upload(D)
        cv = D.ptrs(cj)
        D.call("sfp_modup_prepare", cv, ell, K.KS["K"], K.KS["alpha"])
        tabs[ell] = (cj, cv, cP, KEY)
        handles += cj + [cP]
    return tabs, handles


def case_chain_batch(devs, pset, ells, logn=LOGN):
    """len(ells) key-switch chains in one batch, op i at level ells[i] (ell of Lq = 7, K = 2,
    alpha = 2): sfp_modup, sfp_ks_inner_fold, then sfp_moddown_rescale (even i) or sfp_ks_inner +
    sfp_moddown2 (odd i), then sfp_mult_relin_rescale where the library has it.  Equal levels:
    the same kernels over different rows throughout; mixed levels: the same kernels with
    different row counts, digit counts and tables, and MDRS heads that must not merge.

    Derivation: chain_tokens lists each op's launches; flush_model gives the pair.  Op 0 runs
    once outside the region first, so that the device's constant pool exists (its first
    allocation drains the device, which would flush the region half-way)."""
    R, Ds = K.setup(devs, logn, K.ks_primes(pset, logn))
    n = R.n
    for D in Ds:
        tabs, handles = chain_devices(D, R, ells)
        ops = [ChainOp(D, R, ell, i, tabs[ell]) for i, ell in enumerate(ells)]
        ops[0].issue()
        D.call("sfp_sync")
        ops[0].refill()
        got = run_batch(D, len(ops), [op.issue for op in ops])
        for op in ops:
            ext, out, mrr = chain_exact(pset, op.ell, op.i, logn)
            what = "chain batch %s %s, op %d" % (pset, list(ells), op.i)
            e = D.down(op.E, (op.beta, op.rows, n))
            for j in range(op.beta):
                assert_eq(e[j], ext[j], what + " modup digit %d" % j)
            for p in range(2):
                check_out(D, op.o[p], op.nout, n, out[p], what + (" moddown_rescale" if op.i % 2 == 0 else " moddown2") + " out%d" % p)
                if op.fused:
                    check_out(D, op.m[p], op.ell - 1, n, mrr[p], what + " mult_relin_rescale out%d" % p)
                else:
                    assert (D.down(op.m[p], (op.ell * n,)) == FILL).all(), what + ": a declined mult_relin_rescale wrote"
        assert all(op.fused == D.merges() for op in ops), "sfp_mult_relin_rescale: %s" % [op.fused for op in ops]
        groups = expect(D, got, [chain_tokens(R, op.ell, op.i, op.fused) for op in ops], "chain %s %s" % (pset, list(ells)))
        if groups:
            check_mdrs_groups(groups, ells)
        D.call("sfp_sync")
        for c in handles:
            D.call("sfp_free_conv", c)
        D.release()


def check_mdrs_groups(groups, ells):
    """No MDRS launch of the model joins two levels (the stats then say that the library issued
    exactly the model's launches)."""
    for cls, key, lanes in groups:
        if cls == "MDRS":
            assert len({ells[l] for l in lanes}) == 1, groups


def case_chain_batch_large(devs, ells_rel, logn=16):
    """The same at ring 2^16 (k_modup_col, k_ntt_ks and the mdrs kernels exist only there), setup as
    case_ks_chain_large: op i at level 5 + ells_rel[i] on input i % 2.  A full Python transform is
    too slow here: the reference is the first library's own unbatched sequence (the oracle's on
    the GPU half; that sequence is held to exact arithmetic at 2^12 and spot-checked at 2^16 by
    case_ks_chain_large), plus, for the level-5 ops, the ragged digit's ModUp against the
    definition at the border indices.

    Derivation: as case_chain_batch.  (0, 0): every launch of both ops merges, single = 0.
    (0, 0, -1): the two level-5 ops pair in every class while the level-4 op's MDRS heads find
    no partner (check_mdrs_groups) and issue alone."""
    R, Ds = K.setup(devs, logn, K.ks_primes("fp", logn))
    n = R.n
    ells = [K.KS["ell"] + r for r in ells_rel]
    up5, _ = chain_tables(R, 5)
    spots = {}
    for i in sorted({i % 2 for i, ell in enumerate(ells) if ell == 5}):
        c4 = R.intt(chain_inputs(R, 5, i)[0][4], 4)
        spots[i] = {(r, x): R.ntt_at(c4 % R.primes[p], p, x) for p, r in zip(up5[2].T, up5[2].dst_row)
                    for x in R.border_indices()[::5]}
    first = None
    for D in reversed(Ds):
        tabs, handles = chain_devices(D, R, ells)

        def run(batched):
            ops = [ChainOp(D, R, ell, i % 2, tabs[ell]) for i, ell in enumerate(ells)]
            if batched:
                got = run_batch(D, len(ops), [op.issue for op in ops])
            else:
                for op in ops:
                    op.issue()
                    if not op.fused:
                        op.mrr_unfused()
                got = None
            res = []
            for op in ops:
                res.append((D.down(op.E, (op.beta, op.rows, n)), [D.down(p, (op.nout + 1, n)) for p in op.o],
                            [D.down(p, (op.ell, n)) for p in op.m] if op.fused or not batched else None))
            return ops, got, res
        # every library's unbatched sequence first: the reference (the first library's), and the
        # device's constant pool exists before the region (its first allocation drains the
        # device, which would flush the region half-way)
        _, _, plain = run(False)
        if first is None:
            first = plain
            for i, ell in enumerate(ells):
                if ell == 5:
                    for (r, x), w in spots[i % 2].items():
                        assert int(first[i][0][2, r, x]) == w, ("modup 2^16 ragged digit", i, r, x)
        for i, (a, b) in enumerate(zip(plain, first)):
            assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2])), \
                "chain 2^16 %s, op %d: the libraries' unbatched sequences differ" % (ells, i)
        ops, got, res = run(True)
        for i, (op, (e, o, mm)) in enumerate(zip(ops, res)):
            what = "chain batch 2^16 %s, op %d" % (ells, i)
            assert np.array_equal(e, first[i][0]), what + ": modup differs from the unbatched sequence"
            for p in range(2):
                assert np.array_equal(o[p], first[i][1][p]), what + ": out%d differs from the unbatched sequence" % p
                assert (o[p][op.nout] == FILL).all(), what + ": wrote past its rows"
                if mm is not None:
                    assert np.array_equal(mm[p], first[i][2][p]), what + ": mult_relin_rescale out%d" % p
                    assert (mm[p][op.ell - 1] == FILL).all(), what + ": mult_relin_rescale wrote past its rows"
        assert all(op.fused == D.merges() for op in ops)
        groups = expect(D, got, [chain_tokens(R, op.ell, op.i, op.fused) for op in ops], "chain 2^16 %s" % ells)
        if groups:
            check_mdrs_groups(groups, ells)
            pair = [g for g in groups if g[0] == "MDRS" and g[2] == (0, 1)]
            assert pair, "the model has no merged MDRS pair of ops 0 and 1: %s" % groups
            if len(ells) == 3:
                assert [g for g in groups if g[0] == "MDRS" and g[2] == (2,)], groups
        D.call("sfp_sync")
        for c in handles:
            D.call("sfp_free_conv", c)
        D.release()


# --------------------------------------------------------------------------
# 6. a stacked region over the four real lanes

_lane_ref = {}


def lane_ref(R, l, pt):
    """Lane l's map, input, exact forward NTT and the exact inverse NTT of (forward * pt)."""
    m = maps4()[l]
    a, f, _ = K.ntt_reference(R, m)[NTT_NAMES[l]]
    key = (id(R), l, u64(pt).tobytes())
    if key not in _lane_ref:
        _lane_ref[key] = H.exact_rows(R, m, f * obj(pt) % H.qcol(R, m), R.intt)
    return m, a, f, _lane_ref[key]


def case_stack_lanes(devs, offset, logn=LOGN):
    """Between sfp_stack_begin and sfp_stack_end every lane l of four runs, on its own map
    (9, 4, 5, 1 rows): NTT forward of X_l, Y_l = X_l * PT_l, NTT inverse of Y_l.  offset: lanes
    1 to 3 first form PT_l = U_l + V_l with one leading sfp_add that lane 0 (its PT uploaded)
    does not issue.

    Derivation: without the offset the four lanes' heads agree at every step: forward COL,
    forward ROW, k_ew mul, inverse ROW, inverse COL: (5, 0).  With it the first round's largest
    group is the three adds, after which the four lanes are aligned: (6, 0)."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    lanes_in = []
    for l in range(4):
        m = maps4()[l]
        q = H.qcol(R, m)
        u, v = pp(R, m, 600 + l)["uniform"], pp(R, m, 610 + l)[PATS[l % 3]]
        pt = (u + v) % q if offset and l else u
        lanes_in.append((u, v, pt) + lane_ref(R, l, pt))
    for D in Ds:
        assert D.call("sfp_lanes") >= 4
        bufs = []
        for u, v, pt, m, a, f, w in lanes_in:
            X = out_buf(D, m.count, n)
            D.put(X, u64(a))
            bufs.append((X, out_buf(D, m.count, n), D.up(u64(u)), D.up(u64(v)), out_buf(D, m.count, n)))
        toks = []
        with D.stats_delta() as got:
            D.call("sfp_stack_begin")
            for l, ((u, v, pt, m, a, f, w), (X, Y, U, V, PT)) in enumerate(zip(lanes_in, bufs)):
                D.call("sfp_set_lane", l)
                t = []
                if offset and l:
                    D.call("sfp_add", PT, U, V, m)
                    t += [L("Y", "add")]
                D.call("sfp_ntt", X, m, 0)
                D.call("sfp_mul", Y, X, PT if offset and l else U, m)
                D.call("sfp_ntt", Y, m, 1)
                toks.append(t + t_ntt(m.count, 0) + [L("Y", "mul")] + t_ntt(m.count, 1))
            D.call("sfp_set_lane", 0)
            D.call("sfp_stack_end")
        for l, ((u, v, pt, m, a, f, w), (X, Y, U, V, PT)) in enumerate(zip(lanes_in, bufs)):
            check_out(D, X, m.count, n, f, "stacked lanes: lane %d forward" % l)
            check_out(D, Y, m.count, n, w, "stacked lanes: lane %d product's inverse" % l)
            if offset and l:
                check_out(D, PT, m.count, n, pt, "stacked lanes: lane %d leading add" % l)
        expect(D, got(), toks, "stacked lanes offset=%d" % offset)
        D.release()


def case_stack_events(devs, logn=LOGN):
    """A dependency chain through a stacked region, all on ident(9):
      before the region, lane 0 forms P = A3 * B3 and records event e_pre;
      lane 0: NTT forward of B0 in place, records e0;
      lane 1: waits for e0; Y1 = B0 * X1; then three running sums Y1 += X1 into further buffers;
      lane 2: sfp_lane_wait(2, 1) after lane 1's product; Y2 = Y1 + X2, then five running sums;
      lane 3: waits for e_pre; Y3 = P + X3.
    Lanes 1 and 2 have more items left than the lane they wait for, so "furthest behind first"
    would pick them first if a wait did not hold them: their exact results need the order.

    Derivation: lane 3's add and lane 0's forward COL pass open; the records and waits cost no
    launch; flush_model gives the pair."""
    R, Ds = K.setup(devs, logn)
    n, m = R.n, ident(9)
    q = H.qcol(R, m)
    ref = K.ntt_reference(R, m)
    b0, fb0 = ref["uniform"][0], ref["uniform"][1]
    x1, x2, x3 = (pp(R, m, 700 + j)["uniform"] for j in range(3))
    a3, b3 = pp(R, m, 710)["uniform"], pp(R, m, 711)["alt1"]
    y1 = [fb0 * x1 % q]
    for _ in range(3):
        y1.append((y1[-1] + x1) % q)
    y2 = [(y1[0] + x2) % q]
    for _ in range(5):
        y2.append((y2[-1] + x2) % q)
    p3 = a3 * b3 % q
    for D in Ds:
        B0 = out_buf(D, 9, n)
        D.put(B0, u64(b0))
        X1, X2, X3, A3, B3 = (D.up(u64(x)) for x in (x1, x2, x3, a3, b3))
        P3, Y3 = out_buf(D, 9, n), out_buf(D, 9, n)
        Y1 = [out_buf(D, 9, n) for _ in y1]
        Y2 = [out_buf(D, 9, n) for _ in y2]
        D.call("sfp_set_lane", 0)
        D.call("sfp_mul", P3, A3, B3, m)
        e_pre = D.call("sfp_event_record")
        with D.stats_delta() as got:
            D.call("sfp_stack_begin")
            D.call("sfp_ntt", B0, m, 0)
            e0 = D.call("sfp_event_record")
            D.call("sfp_set_lane", 1)
            D.call("sfp_event_wait", e0)
            D.call("sfp_mul", Y1[0], B0, X1, m)
            D.call("sfp_lane_wait", 2, 1)
            for j in range(1, len(Y1)):
                D.call("sfp_add", Y1[j], Y1[j - 1], X1, m)
            D.call("sfp_set_lane", 2)
            D.call("sfp_add", Y2[0], Y1[0], X2, m)
            for j in range(1, len(Y2)):
                D.call("sfp_add", Y2[j], Y2[j - 1], X2, m)
            D.call("sfp_set_lane", 3)
            D.call("sfp_event_wait", e_pre)
            D.call("sfp_add", Y3, P3, X3, m)
            D.call("sfp_set_lane", 0)
            D.call("sfp_stack_end")
        D.call("sfp_event_free", e0)
        D.call("sfp_event_free", e_pre)
        check_out(D, B0, 9, n, fb0, "stacked events: lane 0 transform")
        for j, (p, w) in enumerate(zip(Y1, y1)):
            check_out(D, p, 9, n, w, "stacked events: lane 1 step %d (after lane 0's record)" % j)
        for j, (p, w) in enumerate(zip(Y2, y2)):
            check_out(D, p, 9, n, w, "stacked events: lane 2 step %d (after lane 1's product)" % j)
        check_out(D, Y3, 9, n, (p3 + x3) % q, "stacked events: lane 3 (after the event before the region)")
        add, mul = L("Y", "add"), L("Y", "mul")
        toks = [t_ntt(9, 0) + [("R", 1)],
                [("W", 1), mul, ("R", 2)] + [add] * 3,   # (sfp_lane_wait records on the waitee ...
                [("W", 2)] + [add] * 6,                  #  ... and waits on the waiter)
                [("W", 0), add]]
        expect(D, got(), toks, "stacked events")
        D.release()


def case_batch_inside_stack(devs, logn=LOGN):
    """sfp_batch_begin inside a stacked region returns 0; sfp_batch_lane and sfp_batch_end are then
    harmless and the two adds issued there run on the caller's lane, in order: (0, 2)."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    specs = [ew_spec(R, "add", i) for i in range(2)]
    for D in Ds:
        bufs = [([out_buf(D, s[0], n)], [D.up(u64(x)) for x in s[2]]) for s in specs]
        with D.stats_delta() as got:
            D.call("sfp_stack_begin")
            assert D.call("sfp_batch_begin", 2) == 0
            for i, (s, b) in enumerate(zip(specs, bufs)):
                D.call("sfp_batch_lane", i)
                s[3](D, b[0], b[1])
            D.call("sfp_batch_end")
            assert D.call("sfp_get_lane") == 0
            D.call("sfp_stack_end")
        for i, (s, b) in enumerate(zip(specs, bufs)):
            check_out(D, b[0][0], s[0], n, s[4][0], "batch inside a stacked region, add %d" % i)
        expect(D, got(), [[L("Y", "add"), L("Y", "add")]], "batch inside a stacked region")
        D.release()


# --------------------------------------------------------------------------
# 7. a host synchronisation inside a batch

def case_sync_inside_batch(devs, logn=LOGN):
    """A batch declared for 8 ops: sfp_mul_add on lanes 0 to 3, then a download of op 0's output --
    a host synchronisation, which flushes what is recorded, so it is already exact -- then ops 4 to
    7 and sfp_batch_end.  Derivation: each half is one group of four: (2, 0)."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    specs = [ew_spec(R, "mul_add", i) for i in range(8)]
    for D in Ds:
        bufs = [([out_buf(D, s[0], n)], [D.up(u64(x)) for x in s[2]]) for s in specs]
        with D.stats_delta() as got:
            assert D.call("sfp_batch_begin", 8) == (1 if D.merges() else 0)
            for i in range(4):
                D.call("sfp_batch_lane", i)
                specs[i][3](D, *bufs[i])
            check_out(D, bufs[0][0][0], specs[0][0], n, specs[0][4][0], "a download in the middle of a batch, op 0")
            for i in range(4, 8):
                D.call("sfp_batch_lane", i)
                specs[i][3](D, *bufs[i])
            D.call("sfp_batch_end")
        for i, (s, b) in enumerate(zip(specs, bufs)):
            check_out(D, b[0][0], s[0], n, s[4][0], "a batch with a download in its middle, op %d" % i)
        toks = [[L("Y", "mul_add")] for _ in range(4)]
        if D.merges():
            m, s, _ = flush_model(toks)
            assert got() == (2 * m, 2 * s) == (2, 0), got()
        else:
            assert got() == (0, 0)
        D.release()


# --------------------------------------------------------------------------
# 8. batches inside a capture

def case_batch_in_capture(devs, logn=LOGN):
    """Libraries with graphs (sfp_capture_begin returns 0; the oracle has none and is skipped): a
    batch of 3 sfp_lin_wsum (nin 1, 5, 80; host weight arrays) and a batch of 2 sfp_ntt are
    captured; then the host weight and pointer arrays are overwritten, and the staging ring
    the weights passed through is recycled by 17 MiB of further unbatched weight uploads.  The
    graph is launched and checked, new inputs are uploaded into the same buffers, and it is
    launched and checked again: the merged launches read the graph's own copies.

    Derivation: (1, 0) for the sums and (2, 0) for the transforms; the graph's nodes are those
    three launches, fewer than the five ops.  Returns the number of libraries that captured."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    ran = 0
    for D in Ds:
        sums = [ew_spec(R, "lin_wsum", i) for i in range(3)]  # maps of 9, 4, 5 rows
        nm = [ident(9), maps4()[2]]
        nref = [K.ntt_reference(R, nm[0]), K.ntt_reference(R, nm[1])]
        souts = [out_buf(D, s[0], n) for s in sums]
        sins = [[D.up(u64(x)) for x in s[2]] for s in sums]
        nbuf = [out_buf(D, m.count, n) for m in nm]
        for p, r in zip(nbuf, nref):
            D.put(p, u64(r["uniform"][0]))
        D.call("sfp_sync")
        if D.call("sfp_capture_begin") != 0:
            D.release()
            continue
        ran += 1
        host = []  # the host arrays of the captured calls

        def wsum(i):
            rows, _, ins, _, _ = sums[i]
            nin = (1, 5, 80)[i]
            polys, k = K.sum_inputs(R, maps4()[i], nin, "half" if nin == 80 else "uniform", 300 + i)
            ptrs, kk = D.ptrs(sins[i] * nin if len(sins[i]) == 1 else sins[i]), u64(k).copy()
            host.extend([ptrs, kk])
            D.call("sfp_lin_wsum", souts[i], ptrs, kk, nin, maps4()[i])
        with D.stats_delta() as got:
            run_batch(D, 3, [lambda i=i: wsum(i) for i in range(3)])
            run_batch(D, 2, [lambda j=j: D.call("sfp_ntt", nbuf[j], nm[j], 0) for j in range(2)])
            g = D.call("sfp_capture_end")
        assert g, "the capture failed"
        assert got() == (3, 0), got()
        nodes = D.call("sfp_graph_nodes", g)
        assert 0 < nodes < 5, nodes
        for a in host:
            a[:] = 0xBAD0BAD0BAD0
        junk_k = np.full((80, 9), 0x123456789, dtype=np.uint64)
        junk_out, junk_in = D.alloc(9 * n), D.ptrs([sins[0][0]] * 80)
        span = (80 * 9 * 8 + 255) & ~255
        for _ in range((17 << 20) // span + 1):
            D.call("sfp_lin_wsum", junk_out, junk_in, junk_k, 80, ident(9))
        for s, p in zip(sums, souts):  # (nothing of the captured region has run)
            assert (D.down(p, ((s[0] + 1) * n,)) == FILL).all(), "a captured launch ran before the replay"
        D.call("sfp_graph_launch", g)
        for i, (s, p) in enumerate(zip(sums, souts)):
            check_out(D, p, s[0], n, s[4][0], "captured batch, lin_wsum %d" % i)
        for j in range(2):
            check_out(D, nbuf[j], nm[j].count, n, nref[j]["uniform"][1], "captured batch, ntt %d" % j)
        # new inputs in the same buffers: the first sum's one input row set and both transforms
        rows0, _, _, _, _ = sums[0]
        _, k0 = K.sum_inputs(R, maps4()[0], 1, "uniform", 300)
        new0 = pp(R, maps4()[0], 900)["uniform"]
        D.put(sins[0][0], u64(new0))
        for j in range(2):
            D.put(nbuf[j], u64(nref[j]["alt1"][0]))
        D.call("sfp_graph_launch", g)
        check_out(D, souts[0], rows0, n, new0 * k0[0].reshape(-1, 1) % H.qcol(R, maps4()[0]), "replay on new inputs, lin_wsum 0")
        for i in (1, 2):
            check_out(D, souts[i], sums[i][0], n, sums[i][4][0], "replay on new inputs, lin_wsum %d" % i)
        for j in range(2):
            check_out(D, nbuf[j], nm[j].count, n, nref[j]["alt1"][1], "replay on new inputs, ntt %d" % j)
        D.call("sfp_graph_destroy", g)
        D.release()
    return ran


# --------------------------------------------------------------------------
# 9. declines

def case_declines(devs, logn=LOGN):
    """sfp_batch_begin returns 0 for count 1 and count 9 on every library, and for count 2 on a
    library that does not merge; sfp_batch_lane and sfp_batch_end are then harmless, two adds
    issued there are exact, and the stats do not move."""
    R, Ds = K.setup(devs, logn)
    n = R.n
    specs = [ew_spec(R, "add", i) for i in range(2)]
    for D in Ds:
        for count in (1, 9) if D.merges() else (1, 9, 2):
            bufs = [([out_buf(D, s[0], n)], [D.up(u64(x)) for x in s[2]]) for s in specs]
            with D.stats_delta() as got:
                assert D.call("sfp_batch_begin", count) == 0, count
                for i, (s, b) in enumerate(zip(specs, bufs)):
                    D.call("sfp_batch_lane", i)
                    s[3](D, b[0], b[1])
                D.call("sfp_batch_end")
            assert D.call("sfp_get_lane") == 0
            for i, (s, b) in enumerate(zip(specs, bufs)):
                check_out(D, b[0][0], s[0], n, s[4][0], "after a declined batch of %d, add %d" % (count, i))
            assert got() == (0, 0), (count, got())
            D.release()


def run_integer_path_cases(devs):
    """Cases 1 to 4 (the fresh SFHE_NTT_FP=0 child of test_gpu_merged_launches.py)."""
    for prim in EW_PRIMS:
        for count in (2, 3, 4, 5, 8):
            case_ew_batch(devs, (prim,), count)
    case_ew_batch(devs, ("add", "mul"), 4)
    for count in range(2, 9):
        case_ntt_batch(devs, "equal", count)
    for count in (4, 7):
        case_ntt_batch(devs, "unequal", count)
    case_ntt_batch(devs, "directions", 4)
    case_ntt_batch_tiles(devs)
    for count in (2, 3, 8):
        case_conv_batch(devs, count)
    for pset in ("mixed", "fp"):
        for count in (2, 3, 4):
            case_chain_batch(devs, pset, [5] * count)
            case_chain_batch(devs, pset, [5, 4, 3, 5][:count])
