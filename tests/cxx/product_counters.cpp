// The engine's relinearised products, one op per case on fresh counters (test
// infrastructure: tests/product_cases.py reads the report).  The C ABI has no
// entry point for EvalMultMany, EvalMultAdd and EvalMultManyAdd, so the cases
// run through the C++ facade, linked against either library.
//   product_counters            every case, one JSON line each
// Ring 2^12, depth 12 (13 limbs), operands at level 10 (ell = 3) and 9 (ell =
// 4), addends at level 11.  SFHE_LAZY, read once per process, selects eager or
// deferred products; the per-call knobs are switched here for the composed
// references.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "openfhe.h"

using namespace lbcrypto;
using CC = CryptoContextImpl<DCRTPoly>;
using Ct = Ciphertext<DCRTPoly>;
using Cts = std::vector<Ct>;

static CryptoContext<DCRTPoly> cc;

static std::string hashOf(const Ct& ct) {
    std::vector<uint64_t> h((size_t)2 * ct->GetNumLimbs() * cc->GetRingDimension());
    cc->DownloadRows(ct, h.data());
    uint64_t f = 1469598103934665603ull;
    for (uint64_t v : h) f = (f ^ v) * 1099511628211ull;
    char buf[40];
    std::snprintf(buf, sizeof buf, "\"L%u:%016llx\"", ct->GetLevel(), (unsigned long long)f);
    return buf;
}

static std::string hashes(const Cts& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + hashOf(v[i]);
    return s + "]";
}

// op on fresh counters, then ref (the same values from separate ops or with the op's knob off)
static void run(const char* name, const std::function<Cts()>& op, const std::function<Cts()>& ref) {
    uint64_t f0[3], f1[3];
    cc->Synchronize();
    cc->ResetOpStats();
    cc->FusedSumCounts(&f0[0], &f0[1], &f0[2]);
    std::string err;
    Cts out;
    try {
        out = op();
    } catch (const OpenFHEException& e) {
        err = e.what();
    }
    const auto s = cc->GetOpStats();
    cc->FusedSumCounts(&f1[0], &f1[1], &f1[2]);
    std::printf("CASE {\"name\": \"%s\", \"counts\": [%llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu], "
                "\"bytes\": %.17g, \"dot\": [%llu, %llu], \"sumn\": [%llu, %llu], \"batches\": [%llu, %llu], "
                "\"folded\": [%llu, %llu, %llu], \"error\": \"%s\", \"hash\": %s, \"ref\": %s}\n",
                name, (unsigned long long)s.keyswitch, (unsigned long long)s.rescale, (unsigned long long)s.tensor,
                (unsigned long long)s.ptmult, (unsigned long long)s.constmult, (unsigned long long)s.add,
                (unsigned long long)s.automorph, (unsigned long long)s.ntt_limbs, (unsigned long long)s.wsum_terms,
                s.algo_bytes, (unsigned long long)s.dot_fused, (unsigned long long)s.dot_composed,
                (unsigned long long)s.sumn_fused, (unsigned long long)s.sumn_composed,
                (unsigned long long)s.sumn_batches, (unsigned long long)s.sumn_fallbacks,
                (unsigned long long)(f1[0] - f0[0]), (unsigned long long)(f1[1] - f0[1]),
                (unsigned long long)(f1[2] - f0[2]), err.c_str(), hashes(out).c_str(),
                hashes(err.empty() && ref ? ref() : Cts{}).c_str());
    std::fflush(stdout);
}

// the value of EvalMultAdd from the separate public ops
static Ct after(Ct prod, const CC::MultAddend& add) {
    if (add.r) prod = add.sign < 0 ? cc->EvalSub(prod, add.r) : cc->EvalAdd(prod, add.r);
    if (add.c != 0.0) prod = cc->EvalAdd(prod, add.c);
    return prod;
}

static Cts knobOffRun(const char* knob, const std::function<Cts()>& op) {
    setenv(knob, "0", 1);
    Cts out = op();
    unsetenv(knob);
    return out;
}

int main() {
    CCParams<CryptoContextCKKSRNS> p;
    p.SetRingDim(1u << 12);
    p.SetMultiplicativeDepth(12);
    p.SetScalingModSize(40);
    p.SetBatchSize(8);
    p.SetSecurityLevel(HEStd_NotSet);
    p.SetSeed(1234);
    cc = GenCryptoContext(p);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    cc->Enable(ADVANCEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    std::mt19937_64 rng(5);
    auto fresh = [&](uint32_t level) {
        std::vector<double> v(8);
        for (double& x : v) x = (double)(rng() % 2001) / 1000.0 - 1.0;
        return cc->Encrypt(kp.publicKey, cc->MakeCKKSPackedPlaintext(v, 1, level, nullptr, 8));
    };
    Cts c, d;
    for (int i = 0; i < 8; ++i) c.push_back(fresh(10));
    for (int i = 0; i < 4; ++i) d.push_back(fresh(9));
    const Ct r = fresh(11), r2 = fresh(11);
    Ct odd = r2->Clone();  // (the right level under another scale label: never folded)
    odd->scale *= 0.5;
    using Add = CC::MultAddend;
    using Term = CC::MultTerm;
    using Op = CC::MultSumOp;

    run("mult", [&] { return Cts{cc->EvalMult(c[0], c[1])}; }, nullptr);
    {
        const Cts a{c[0], c[2], c[4]}, b{c[1], c[3], c[5]};
        run("mult_many_one_level", [&] { return cc->EvalMultMany(a, b); },
            [&] { return Cts{cc->EvalMult(a[0], b[0]), cc->EvalMult(a[1], b[1]), cc->EvalMult(a[2], b[2])}; });
    }
    {
        const Cts a{c[0], d[0], d[2]}, b{c[1], d[1], d[3]};
        run("mult_many_two_levels", [&] { return cc->EvalMultMany(a, b); },
            [&] { return Cts{cc->EvalMult(a[0], b[0]), cc->EvalMult(a[1], b[1]), cc->EvalMult(a[2], b[2])}; });
    }
    const std::pair<const char*, Add> single[] = {{"mult_add_ciphertext", Add{r, -1, 0.0}},
                                                  {"mult_add_constant", Add{nullptr, 1, 0.25}},
                                                  {"mult_add_both", Add{r, 1, 0.25}}};
    for (const auto& [name, add] : single) {
        const Add ad = add;
        run(name, [&] { return Cts{cc->EvalMultAdd(c[0], c[1], ad)}; },
            [&] { return Cts{after(cc->EvalMult(c[0], c[1]), ad)}; });
    }
    {
        const Cts a{c[0], c[2], c[4]}, b{c[1], c[3], c[5]};
        const std::vector<Add> adds{Add{r, 1, 0.0}, Add{odd, 1, 0.0}, Add{nullptr, 1, 0.5}};
        run("mult_many_add", [&] { return cc->EvalMultManyAdd(a, b, adds); }, [&] {
            Cts out;
            for (size_t i = 0; i < 3; ++i) out.push_back(after(cc->EvalMult(a[i], b[i]), adds[i]));
            return out;
        });
    }
    for (int with = 1; with >= 0; --with) {
        auto op = [&] { return Cts{cc->EvalMultSum2(c[0], c[1], c[2], c[3], with ? r : nullptr)}; };
        run(with ? "mult_sum2_addend" : "mult_sum2", op, [&] { return knobOffRun("SFHE_MULT_SUM2_FUSED", op); });
    }
    const std::vector<Term> t3{{c[0], c[1]}, {c[2], c[3]}, {c[4], c[5]}};
    const Add sumAdd[] = {Add{r, 1, 0.0}, Add{r, -1, 0.25}, Add{}};
    for (size_t m = 1; m <= 3; ++m) {
        const std::string name = "mult_sum_" + std::to_string(m);
        auto op = [&] { return Cts{cc->EvalMultSum(std::vector<Term>(t3.begin(), t3.begin() + m), sumAdd[m - 1])}; };
        run(name.c_str(), op, [&] { return knobOffRun("SFHE_MULT_SUM_FUSED", op); });
    }
    {
        const std::vector<Op> ops{Op{{t3[0], t3[1]}, Add{r, 1, 0.0}}, Op{{t3[1], t3[2]}, Add{}},
                                  Op{{t3[0], t3[1], t3[2]}, Add{}}, Op{{t3[2], t3[0]}, Add{}}};
        auto op = [&] { return cc->EvalMultSumMany(ops); };
        run("mult_sum_many", op, [&] { return knobOffRun("SFHE_MULT_SUM_FUSED", op); });
    }
    // an addend one level too high: each op throws under its own name
    run("mult_sum2_wrong_level", [&] { return Cts{cc->EvalMultSum2(c[0], c[1], c[2], c[3], c[4])}; }, nullptr);
    run("mult_sum_wrong_level", [&] { return Cts{cc->EvalMultSum({t3[0], t3[1]}, Add{c[4], 1, 0.0})}; }, nullptr);
    cc->Synchronize();
    return 0;
}
