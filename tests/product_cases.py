"""The engine's relinearised products, one op per case on fresh counters: what each op counts.

tests/cxx/product_counters.cpp runs the cases through the C++ facade (the C ABI has no entry
point for EvalMultMany, EvalMultAdd and EvalMultManyAdd) and reports, per case, the op_stats
delta with the byte model's figure, the dot / sumn / batch counters, the sums folded into a
product's last pass (FusedSumCounts) and a hash of every result's residues, next to the hash of
the same values formed by separate public ops or with the op's knob off.

The expectations below are written out from context.cpp's counting rules, never read back:
  a tensor                     tensor + 1,               7 l words per coefficient
  a relinearisation + rescale  keyswitch + 1, rescale + 1, 3 l + 2 beta (l + K) and 4 l
  a sum of two ciphertexts     add + 1,                  6 l' (l' = l - 1: the result's limbs)
  a sum with a constant        add + 1,                  4 l'
  EvalMultSum / Sum2           add + 1 for the tensors' sum when m > 1
A sum the backend folds into the product counts as the EvalAdd it replaces, with one exception
the engine keeps: EvalMultSum2's fused form counts its addend in `add` but charges no bytes for
it.  Ring 2^12, 13 limbs, operands at level 10 (l = 3, one digit) and 9 (l = 4), so n = 4096
coefficients of 8 bytes; K is the special-prime count of the level's key (special_primes()).
"""
import json
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cxx"))
import reference_harness as RH  # noqa: E402

N, DEPTH, SEED = 1 << 12, 12, 1234
W = N * 8  # bytes per limb row


def special_primes(primes, Lq, K, alpha, ell, spec=(2, 4, 6, 8, 10)):
    """K of the key a switch at ell limbs uses: buildTiers' rule restated (the first K' special
    primes whose product has 20 bits over the first b limbs', kept when K' + 1 < K and K' grows)."""
    tiers = []
    for b in spec:
        if b > alpha or b > Lq:
            break
        bits = sum(math.log2(p) for p in primes[:b])
        k, bp = 0, 0.0
        while bp < bits + 20.0 and k < K:
            bp += math.log2(primes[Lq + k])
            k += 1
        if k + 1 >= K or (tiers and k <= tiers[-1][1]):
            continue
        tiers.append((b, k))
    return next((k for b, k in tiers if ell <= b), K)


def expected(backend, lazy, K3, K4):
    """name -> dict of the fields product_counters.cpp reports (counts: keyswitch, rescale, tensor,
    ptmult, constmult, add, automorph, ntt_limbs, wsum_terms)."""
    hip = backend == "hip"
    T3, T4 = 7 * 3 * W, 7 * 4 * W
    R3 = (3 * 3 + 2 * (3 + K3)) * W + 4 * 3 * W  # (beta = 1: one digit)
    R4 = (3 * 4 + 2 * (4 + K4)) * W + 4 * 4 * W
    ADD, ADDC = 6 * 2 * W, 4 * 2 * W  # at the results' level 11: two limbs

    def case(ks, tensor, add, nbytes, dot=(0, 0), sumn=(0, 0), batches=(0, 0), folded=(0, 0, 0), error=""):
        return dict(counts=[ks, ks, tensor, 0, 0, add, 0, 0, 0], bytes=float(nbytes), dot=list(dot), sumn=list(sumn),
                    batches=list(batches), folded=list(folded), error=error)

    def kind(n):  # (fused, composed): the oracle has no fused form
        return (n, 0) if hip else (0, n)

    fold = hip and not lazy  # a lazy context forms the product first, then the separate sums
    E = {
        # a deferred product counts its tensor now and its relinearisation where it is computed
        "mult": case(0, 1, 0, T3) if lazy else case(1, 1, 0, T3 + R3),
        "mult_many_one_level": case(3, 3, 0, 3 * (T3 + R3)),
        "mult_many_two_levels": case(3, 3, 0, T3 + R3 + 2 * (T4 + R4)),
        "mult_add_ciphertext": case(1, 1, 1, T3 + R3 + ADD, folded=(1, 0, 0) if fold else (0, 0, 0)),
        "mult_add_constant": case(1, 1, 1, T3 + R3 + ADDC, folded=(0, 1, 0) if fold else (0, 0, 0)),
        "mult_add_both": case(1, 1, 2, T3 + R3 + ADD + ADDC, folded=(1, 1, 0) if fold else (0, 0, 0)),
        # the middle addend carries another scale label: its sum is a separate EvalAdd everywhere
        "mult_many_add": case(3, 3, 3, 3 * (T3 + R3) + 2 * ADD + ADDC, folded=(1, 1, 0) if fold else (0, 0, 0)),
        "mult_sum2_addend": case(1, 2, 2, 2 * T3 + R3 + (0 if hip else ADD), dot=kind(1)),
        "mult_sum2": case(1, 2, 1, 2 * T3 + R3, dot=kind(1)),
        "mult_sum_1": case(1, 1, 1, T3 + R3 + ADD, sumn=kind(1), batches=(1, 0), folded=(1, 0, 0) if hip else (0, 0, 0)),
        "mult_sum_2": case(1, 2, 3, 2 * T3 + R3 + ADD + ADDC, sumn=kind(1), batches=(1, 0),
                           folded=(1, 1, 0) if hip else (0, 0, 0)),
        "mult_sum_3": case(1, 3, 1, 3 * T3 + R3, sumn=kind(1), batches=(1, 0)),
        # term counts 2, 2, 3, 2: three runs; nine tensors, four sums of tensors, one addend
        "mult_sum_many": case(4, 9, 5, 9 * T3 + 4 * R3 + ADD, sumn=kind(4), batches=(3, 0),
                              folded=(1, 0, 0) if hip else (0, 0, 0)),
        "mult_sum2_wrong_level": case(0, 0, 0, 0, error="EvalMultSum2: EvalMultSum2: the addend is not canonical at the "
                                                        "result's level 11"),
        "mult_sum_wrong_level": case(0, 0, 0, 0, error="EvalMultSumMany: EvalMultSum: the addend is not canonical at the "
                                                       "result's level"),
    }
    return E


RESULTS = {"mult": 1, "mult_many_one_level": 3, "mult_many_two_levels": 3, "mult_many_add": 3, "mult_sum_many": 4,
           "mult_sum2_wrong_level": 0, "mult_sum_wrong_level": 0}  # results per case (default 1)
NAMES = list(expected("oracle", False, 0, 0))


def report(backend, lazy):
    """Every case of product_counters_<backend> in one child process: name -> reported fields."""
    exe = RH.build_own([backend])[("product_counters", backend)]  # (the oracle alone suffices without a GPU)
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("SFHE_"):
            del env[k]
    if not lazy:
        env["SFHE_LAZY"] = "0"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            c = json.loads(line[5:])
            out[c.pop("name")] = c
    assert list(out) == NAMES
    return out


def key_sizes(engine):
    """(K at 3 limbs, K at 4 limbs) from the context's own prime chain."""
    info, primes = engine.info(), engine.primes()
    Lq, K = info["num_q"], info["num_p"]
    alpha = -(-Lq // info["dnum"])
    # the expectations take beta = 1 at 3 and 4 limbs, which holds for the default digit count
    # (dnum = 3: alpha = 5); a context built with another SFHE_DNUM needs them rederived
    assert Lq == DEPTH + 1 and alpha >= 4
    return tuple(special_primes(primes, Lq, K, alpha, ell) for ell in (3, 4))


def check(got, want, name):
    """One case's report against the written-out expectation; returns its result hashes."""
    g = got[name]
    for field, v in want[name].items():
        assert g[field] == v, (name, field, g[field], v)
    assert len(g["hash"]) == RESULTS.get(name, 1)
    if g["ref"]:  # the op's values equal the separately formed ones, residue for residue
        assert g["hash"] == g["ref"], name
    assert all(h.startswith("L11:" if "two_levels" not in name or i == 0 else "L10:") for i, h in enumerate(g["hash"]))
    return g["hash"]
