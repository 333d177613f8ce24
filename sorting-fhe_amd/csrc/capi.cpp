// extern "C" boundary (include/sfhe.h) over the lbcrypto-compatible engine.
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <sstream>
#include <streambuf>
#include <string>

#include "../../include/sfhe.h"
#include "algo/coefficients.h"
#include "algo/comparison.h"
#include "algo/encryption.h"
#include "algo/rotation.h"
#include "algo/sign.h"
#include "algo/sort_algo.h"
#include "algo/kway_adapter.h"
#include "core/openfhe.h"
#include "core/state.h"

using namespace lbcrypto;
using Ct = Ciphertext<DCRTPoly>;

struct sfhe_ctx {
    CryptoContext<DCRTPoly> cc;
    KeyPair<DCRTPoly> keys;
    bool quiet = false;
};
struct sfhe_ct {
    Ct ct;
};

namespace {

thread_local std::string g_err;

struct NullBuf : std::streambuf {
    int overflow(int c) override { return c; }
};

// silences std::cout while alive (reference prints inside sort()).  Contexts
// may sort concurrently from several threads (one per lane or per shard rank),
// so the swap is reference-counted under a lock with one shared null buffer:
// a per-object buffer restored out of order would leave std::cout pointing at
// a destroyed stack object.
std::mutex g_quietMu;
int g_quietDepth = 0;
std::streambuf* g_quietOld = nullptr;
NullBuf g_nullBuf;

struct Quiet {
    bool on;
    explicit Quiet(bool q) : on(q) {
        if (!on) return;
        std::lock_guard<std::mutex> g(g_quietMu);
        if (g_quietDepth++ == 0) g_quietOld = std::cout.rdbuf(&g_nullBuf);
    }
    ~Quiet() {
        if (!on) return;
        std::lock_guard<std::mutex> g(g_quietMu);
        if (--g_quietDepth == 0) std::cout.rdbuf(g_quietOld);
    }
};

template <class F>
int guard(F&& f) {
    try {
        f();
        return SFHE_OK;
    } catch (const OpenFHEException& e) {
        g_err = e.what();
        return std::string(e.what()).find("device") != std::string::npos ? SFHE_EDEVICE
                                                                          : SFHE_ESCHEME;
    } catch (const std::invalid_argument& e) {
        g_err = e.what();
        return SFHE_EINVAL;
    } catch (const std::exception& e) {
        g_err = e.what();
        return SFHE_ESCHEME;
    }
}

#define REQUIRE(cond, msg)                    \
    do {                                      \
        if (!(cond)) {                        \
            g_err = msg;                      \
            return SFHE_EINVAL;               \
        }                                     \
    } while (0)

sfhe_ct* wrap(Ct c) { return new sfhe_ct{std::move(c)}; }

SignConfig cfgOf(int n, int dg, int df) { return SignConfig(CompositeSignConfig(n, dg, df)); }

struct SorterBase {
    virtual ~SorterBase() = default;
    virtual uint32_t size() const = 0;
    virtual Ct sort(const Ct& in, SignConfig& cfg) = 0;
    virtual Ct rank(const Ct& in, SignConfig& cfg) = 0;
    virtual Ct sortStable(const Ct& in, SignConfig& cfg) = 0;
    virtual Ct rankStable(const Ct& in, SignConfig& cfg) = 0;
    virtual Ct place(const Ct& rank, const Ct& in) = 0;
    virtual std::vector<Ct> placeMany(const Ct& rank, const std::vector<Ct>& cols) = 0;
    virtual std::vector<Ct> sortRecords(const Ct& keys, const std::vector<Ct>& cols, SignConfig& cfg, bool stable) = 0;
    virtual size_t recordsGraphNodes() const = 0;
    virtual Ct selectRanks(const Ct& rank, const Ct& in, const std::vector<int>& targets) = 0;
    virtual Ct select(const Ct& in, const std::vector<int>& targets, SignConfig& cfg, bool stable) = 0;
    virtual std::vector<Ct> selectRanksMany(const Ct& rank, const std::vector<Ct>& cols,
                                            const std::vector<int>& targets) = 0;
    virtual std::vector<Ct> selectRecords(const Ct& keys, const std::vector<Ct>& cols, const std::vector<int>& targets,
                                          SignConfig& cfg, bool stable) = 0;
    virtual Ct rankLex(const std::vector<Ct>& keys, const std::vector<bool>& desc, SignConfig& cfg) = 0;
    virtual std::vector<Ct> sortRecordsLex(const std::vector<Ct>& keys, const std::vector<Ct>& cols,
                                           const std::vector<bool>& desc, SignConfig& cfg) = 0;
    virtual std::vector<Ct> selectRecordsLex(const std::vector<Ct>& keys, const std::vector<Ct>& cols,
                                             const std::vector<int>& targets, const std::vector<bool>& desc,
                                             SignConfig& cfg) = 0;
    // {count, index (null unless asked for), sums...}
    virtual std::vector<Ct> group(const Ct& keys, const std::vector<Ct>& cols, SignConfig& cfg, bool wantIndex) = 0;
    // {count (null unless asked for), sums...}
    // {count, sums...}
    virtual std::vector<Ct> join(const std::vector<Ct>& keysA, const std::vector<Ct>& keysB,
                                 const std::vector<Ct>& colsB, SignConfig& cfg) = 0;
    virtual std::vector<Ct> window(const Ct& keys, const std::vector<Ct>& cols, SignConfig& cfg, int frame,
                                   bool wantCount) = 0;
    virtual Ct hybrid1(const Ct& in, SignConfig& cfg, const PrivateKey<DCRTPoly>& sk) = 0;
    virtual Ct hybrid(const Ct& in, SignConfig& cfg, const PrivateKey<DCRTPoly>& sk, int variant) = 0;
    virtual Ct place2N(const Ct& rank, const Ct& in) = 0;
    virtual Ct bitonic(const Ct& in, SignConfig& cfg) = 0;
    virtual size_t graphNodes() const = 0;
    virtual bool graphFamilyTime(uint32_t family, int reps, double* ms, uint64_t* launches, double* bytes) = 0;
};

template <int N>
struct Sorter : SorterBase {
    DirectSort<N> ds;
    std::unique_ptr<BitonicSort<N>> bs;  // built on first use (its mask memo lives across sorts)
    CryptoContext<DCRTPoly> cc_;
    PublicKey<DCRTPoly> pk_;
    std::vector<int> rot_;
    std::shared_ptr<Encryption> enc_;
    Sorter(CryptoContext<DCRTPoly> cc, PublicKey<DCRTPoly> pk, std::vector<int> rot,
           std::shared_ptr<Encryption> enc)
        : ds(cc, pk, rot, enc), cc_(cc), pk_(pk), rot_(rot), enc_(enc) {}
    Ct bitonic(const Ct& in, SignConfig& cfg) override {
        if (!bs) bs = std::make_unique<BitonicSort<N>>(cc_, pk_, rot_, enc_);
        return bs->sort(in, SignFunc::CompositeSign, cfg);
    }
    uint32_t size() const override { return (uint32_t)N; }
    Ct sort(const Ct& in, SignConfig& cfg) override { return ds.sort(in, SignFunc::CompositeSign, cfg); }
    Ct rank(const Ct& in, SignConfig& cfg) override {
        return ds.constructRank(in, SignFunc::CompositeSign, cfg);
    }
    Ct sortStable(const Ct& in, SignConfig& cfg) override {
        return ds.sortStable(in, SignFunc::CompositeSign, cfg);
    }
    Ct rankStable(const Ct& in, SignConfig& cfg) override {
        return ds.constructRankStable(in, SignFunc::CompositeSign, cfg);
    }
    Ct place(const Ct& r, const Ct& in) override { return ds.rotationIndexCheckN(r, in); }
    std::vector<Ct> placeMany(const Ct& r, const std::vector<Ct>& cols) override { return ds.placeMany(r, cols); }
    std::vector<Ct> sortRecords(const Ct& keys, const std::vector<Ct>& cols, SignConfig& cfg, bool stable) override {
        return ds.sortRecords(keys, cols, SignFunc::CompositeSign, cfg, stable);
    }
    size_t recordsGraphNodes() const override { return ds.recordsGraphNodes(); }
    Ct selectRanks(const Ct& r, const Ct& in, const std::vector<int>& targets) override {
        return ds.selectRanks(r, in, targets);
    }
    Ct select(const Ct& in, const std::vector<int>& targets, SignConfig& cfg, bool stable) override {
        return ds.select(in, targets, SignFunc::CompositeSign, cfg, stable);
    }
    std::vector<Ct> selectRanksMany(const Ct& r, const std::vector<Ct>& cols,
                                    const std::vector<int>& targets) override {
        return ds.selectRanksMany(r, cols, targets);
    }
    std::vector<Ct> selectRecords(const Ct& keys, const std::vector<Ct>& cols, const std::vector<int>& targets,
                                  SignConfig& cfg, bool stable) override {
        return ds.selectRecords(keys, cols, targets, SignFunc::CompositeSign, cfg, stable);
    }
    Ct rankLex(const std::vector<Ct>& keys, const std::vector<bool>& desc, SignConfig& cfg) override {
        return ds.constructRankLex(keys, desc, SignFunc::CompositeSign, cfg);
    }
    std::vector<Ct> sortRecordsLex(const std::vector<Ct>& keys, const std::vector<Ct>& cols,
                                   const std::vector<bool>& desc, SignConfig& cfg) override {
        return ds.sortRecordsLex(keys, cols, desc, SignFunc::CompositeSign, cfg, SFHE_MAX_COLUMNS);
    }
    std::vector<Ct> selectRecordsLex(const std::vector<Ct>& keys, const std::vector<Ct>& cols,
                                     const std::vector<int>& targets, const std::vector<bool>& desc,
                                     SignConfig& cfg) override {
        return ds.selectRecordsLex(keys, cols, targets, desc, SignFunc::CompositeSign, cfg, SFHE_MAX_COLUMNS);
    }
    std::vector<Ct> group(const Ct& keys, const std::vector<Ct>& cols, SignConfig& cfg, bool wantIndex) override {
        auto r = ds.groupAggregate(keys, cols, SignFunc::CompositeSign, cfg, wantIndex, SFHE_MAX_COLUMNS);
        std::vector<Ct> out{r.count, r.index};
        out.insert(out.end(), r.sums.begin(), r.sums.end());
        return out;
    }
    std::vector<Ct> join(const std::vector<Ct>& keysA, const std::vector<Ct>& keysB, const std::vector<Ct>& colsB,
                         SignConfig& cfg) override {
        auto r = ds.joinAggregate(keysA, keysB, colsB, SignFunc::CompositeSign, cfg, SFHE_MAX_COLUMNS);
        std::vector<Ct> out{r.count};
        out.insert(out.end(), r.sums.begin(), r.sums.end());
        return out;
    }
    std::vector<Ct> window(const Ct& keys, const std::vector<Ct>& cols, SignConfig& cfg, int frame,
                           bool wantCount) override {
        auto r = ds.windowSums(keys, cols, SignFunc::CompositeSign, cfg, frame, wantCount, SFHE_MAX_COLUMNS);
        std::vector<Ct> out{r.count};
        out.insert(out.end(), r.sums.begin(), r.sums.end());
        return out;
    }
    Ct hybrid1(const Ct& in, SignConfig& cfg, const PrivateKey<DCRTPoly>& sk) override {
        return ds.sort_hybrid1(in, SignFunc::CompositeSign, cfg, sk);
    }
    Ct hybrid(const Ct& in, SignConfig& cfg, const PrivateKey<DCRTPoly>& sk, int variant) override {
        return variant == 2 ? ds.sort_hybrid2(in, SignFunc::CompositeSign, cfg, sk)
                            : ds.sort_hybrid(in, SignFunc::CompositeSign, cfg, sk);
    }
    Ct place2N(const Ct& r, const Ct& in) override { return ds.rotationIndexCheck2N(r, in); }
    size_t graphNodes() const override { return ds.graphNodes(); }
    bool graphFamilyTime(uint32_t family, int reps, double* ms, uint64_t* launches, double* bytes) override {
        return ds.graphFamilyTime(family, reps, ms, launches, bytes);
    }
};

template <int N>
int decomposeN(const std::vector<int>& keys, int r, int wrap, int algo, int32_t* v, int32_t* s,
               size_t cap, size_t* count) {
    Decomposer<N> d(keys);
    auto steps = d.decompose(r, wrap, algo == 0 ? DecomposeAlgo::NAF
                                      : algo == 1 ? DecomposeAlgo::BNAF
                                                  : DecomposeAlgo::BINARY);
    if (count) *count = steps.size();
    for (size_t i = 0; i < steps.size() && i < cap; ++i) {
        v[i] = steps[i].value;
        s[i] = steps[i].stepSize;
    }
    return SFHE_OK;
}

bool validN(uint32_t N) {
    return N >= 4 && N <= 1024 && (N & (N - 1)) == 0;
}

}  // namespace

struct sfhe_sorter {
    sfhe_ctx* ctx;
    std::unique_ptr<SorterBase> impl;
};

extern "C" {

int sfhe_abi_version(void) { return SFHE_ABI_VERSION; }
const char* sfhe_last_error(void) { return g_err.c_str(); }
const char* sfhe_backend(void) { return sfp_backend_name(); }

void sfhe_params_default(sfhe_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->mult_depth = 1;
    p->scaling_mod_size = 40;
    p->first_mod_size = 60;
    p->security_level = SFHE_HESTD_128_CLASSIC;
    p->seed = 0x5eed5eed2025ULL;
    p->scaling_technique = SFHE_FLEXIBLEAUTOEXT;
}

int sfhe_context_create(const sfhe_params* p, sfhe_ctx** out) {
    REQUIRE(p && out, "null argument");
    return guard([&] {
        CCParams<CryptoContextCKKSRNS> P;
        P.SetMultiplicativeDepth(p->mult_depth);
        P.SetScalingModSize(p->scaling_mod_size);
        P.SetFirstModSize(p->first_mod_size ? p->first_mod_size : 60);
        P.SetBatchSize(p->batch_size);
        P.SetRingDim(p->ring_dim);
        P.SetSecurityLevel(p->security_level == SFHE_HESTD_NOTSET ? HEStd_NotSet : HEStd_128_classic);
        P.SetNumLargeDigits(p->num_large_digits);
        P.SetDevice(p->device);
        P.SetSeed(p->seed);
        if (p->scaling_technique != 0 && p->scaling_technique != SFHE_FLEXIBLEAUTO &&
            p->scaling_technique != SFHE_FLEXIBLEAUTOEXT)
            throw std::invalid_argument("scaling_technique must be FLEXIBLEAUTO or FLEXIBLEAUTOEXT");
        P.SetScalingTechnique(p->scaling_technique == SFHE_FLEXIBLEAUTO ? FLEXIBLEAUTO
                                                                         : FLEXIBLEAUTOEXT);
        auto c = std::make_unique<sfhe_ctx>();
        c->cc = GenCryptoContext(P);
        c->cc->Enable(PKE);
        c->cc->Enable(KEYSWITCH);
        c->cc->Enable(LEVELEDSHE);
        c->cc->Enable(ADVANCEDSHE);
        *out = c.release();
    });
}

void sfhe_context_destroy(sfhe_ctx* c) { delete c; }

int sfhe_keygen(sfhe_ctx* c) {
    REQUIRE(c, "null context");
    return guard([&] {
        c->keys = c->cc->KeyGen();
        c->cc->EvalMultKeyGen(c->keys.secretKey);
    });
}

int sfhe_rotate_keygen(sfhe_ctx* c, const int32_t* idx, size_t count) {
    REQUIRE(c && (idx || !count), "null argument");
    REQUIRE(c->keys.secretKey, "sfhe_keygen must be called first");
    return guard([&] { c->cc->EvalRotateKeyGen(c->keys.secretKey, std::vector<int32_t>(idx, idx + count)); });
}

int sfhe_context_info(sfhe_ctx* c, uint32_t* n, uint32_t* depth, uint32_t* nq, uint32_t* np,
                      uint32_t* dnum) {
    REQUIRE(c, "null context");
    const SfheContextState* s = c->cc->state();
    if (n) *n = s->n;
    if (depth) *depth = s->L;
    if (nq) *nq = s->Lq;
    if (np) *np = s->K;
    if (dnum) *dnum = s->dnum;
    return SFHE_OK;
}

int sfhe_set_plaintext_cache(sfhe_ctx* c, int on) {
    REQUIRE(c, "null context");
    return guard([&] { c->cc->SetPlaintextCache(on != 0); });
}

int sfhe_set_quiet(sfhe_ctx* c, int q) {
    REQUIRE(c, "null context");
    c->quiet = q != 0;
    return SFHE_OK;
}

int sfhe_sync(sfhe_ctx* c) {
    REQUIRE(c, "null context");
    return guard([&] { c->cc->Synchronize(); });
}

int sfhe_op_stats(sfhe_ctx* c, uint64_t* counts, double* bytes, int reset) {
    REQUIRE(c, "null context");
    auto s = c->cc->GetOpStats();
    if (counts) {
        uint64_t v[9] = {s.keyswitch, s.rescale, s.tensor,  s.ptmult,    s.constmult,
                         s.add,       s.automorph, s.ntt_limbs, s.wsum_terms};
        std::memcpy(counts, v, sizeof v);
    }
    if (bytes) *bytes = s.algo_bytes;
    if (reset) c->cc->ResetOpStats();
    return SFHE_OK;
}

int sfhe_bootstrap_graphs(sfhe_ctx* c, uint64_t* count) {
    REQUIRE(c && count, "null argument");
    *count = c->cc->BootstrapGraphs();
    return SFHE_OK;
}

int sfhe_encode_counts(sfhe_ctx* c, uint64_t* device, uint64_t* host) {
    REQUIRE(c && device && host, "null argument");
    auto s = c->cc->GetOpStats();
    *device = s.dev_encodes;
    *host = s.host_encodes;
    return SFHE_OK;
}

int sfhe_encrypt(sfhe_ctx* c, const double* v, size_t len, uint32_t slots, uint32_t level,
                 sfhe_ct** out) {
    REQUIRE(c && out && (v || !len), "null argument");
    REQUIRE(c->keys.publicKey, "sfhe_keygen must be called first");
    return guard([&] {
        auto pt = c->cc->MakeCKKSPackedPlaintext(std::vector<double>(v, v + len), 1, level, nullptr, slots);
        *out = wrap(c->cc->Encrypt(c->keys.publicKey, pt));
    });
}

int sfhe_encrypt_batch(sfhe_ctx* c, const double* values, size_t stride, const size_t* lens, size_t count,
                       uint32_t slots, const uint32_t* levels, sfhe_ct** outs) {
    REQUIRE(c && (outs || !count) && (lens || !count), "null argument");
    REQUIRE(c->keys.publicKey, "sfhe_keygen must be called first");
    for (size_t k = 0; k < count; ++k) {
        REQUIRE(lens[k] <= stride, "an input longer than the stride");
        REQUIRE(values || !lens[k], "null values");
    }
    return guard([&] {
        std::vector<Plaintext> pts(count);
        for (size_t k = 0; k < count; ++k) {
            const double* v = lens[k] ? values + k * stride : nullptr;
            pts[k] = c->cc->MakeCKKSPackedPlaintext(std::vector<double>(v, v + lens[k]), 1, levels ? levels[k] : 0,
                                                    nullptr, slots);
        }
        auto cts = c->cc->EncryptMany(c->keys.publicKey, pts);
        for (size_t k = 0; k < count; ++k) outs[k] = wrap(cts[k]);
    });
}

int sfhe_sample_counts(sfhe_ctx* c, uint64_t* device, uint64_t* host) {
    REQUIRE(c && device && host, "null argument");
    auto s = c->cc->GetOpStats();
    *device = s.dev_samples;
    *host = s.host_samples;
    return SFHE_OK;
}

int sfhe_decrypt(sfhe_ctx* c, const sfhe_ct* ct, double* out, size_t cap, size_t* len) {
    REQUIRE(c && ct, "null argument");
    REQUIRE(c->keys.secretKey, "no secret key");
    return guard([&] {
        Plaintext pt;
        c->cc->Decrypt(c->keys.secretKey, ct->ct, &pt);
        const auto& v = pt->GetRealPackedValue();
        if (len) *len = v.size();
        for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    });
}

int sfhe_decrypt_batch(sfhe_ctx* c, const sfhe_ct* const* cts, size_t count, double* out, size_t stride,
                       size_t* lens) {
    REQUIRE(c && (cts || !count), "null argument");
    REQUIRE(out || !stride || !count, "null output with a non-zero stride");
    REQUIRE(c->keys.secretKey, "no secret key");
    for (size_t k = 0; k < count; ++k) REQUIRE(cts[k], "null ciphertext");
    return guard([&] {
        std::vector<Ciphertext<DCRTPoly>> in(count);
        for (size_t k = 0; k < count; ++k) in[k] = cts[k]->ct;
        std::vector<Plaintext> pts;
        c->cc->DecryptMany(c->keys.secretKey, in, &pts);
        for (size_t k = 0; k < count; ++k) {
            const auto& v = pts[k]->GetRealPackedValue();
            if (lens) lens[k] = v.size();
            for (size_t i = 0; i < v.size() && i < stride; ++i) out[k * stride + i] = v[i];
        }
    });
}

int sfhe_decode_counts(sfhe_ctx* c, uint64_t* device, uint64_t* host) {
    REQUIRE(c && device && host, "null argument");
    auto s = c->cc->GetOpStats();
    *device = s.dev_decodes;
    *host = s.host_decodes;
    return SFHE_OK;
}

int sfhe_tie_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.tie_fused;
    *composed = s.tie_composed;
    return SFHE_OK;
}

int sfhe_lex_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.lex_fused;
    *composed = s.lex_composed;
    return SFHE_OK;
}

int sfhe_dot_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.dot_fused;
    *composed = s.dot_composed;
    return SFHE_OK;
}

int sfhe_sumn_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.sumn_fused;
    *composed = s.sumn_composed;
    return SFHE_OK;
}

int sfhe_sumn_batch_counts(sfhe_ctx* c, uint64_t* batches, uint64_t* fallbacks) {
    REQUIRE(c && batches && fallbacks, "null argument");
    auto s = c->cc->GetOpStats();
    *batches = s.sumn_batches;
    *fallbacks = s.sumn_fallbacks;
    return SFHE_OK;
}

int sfhe_group_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.gate_fused;
    *composed = s.gate_composed;
    return SFHE_OK;
}

int sfhe_window_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.weight_fused;
    *composed = s.weight_composed;
    return SFHE_OK;
}

int sfhe_join_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *fused = s.or_fused;
    *composed = s.or_composed;
    return SFHE_OK;
}

int sfhe_place_counts(sfhe_ctx* c, uint64_t* hits, uint64_t* columns, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && hits && columns && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *hits = s.place_hits;
    *columns = s.place_columns;
    *fused = s.place_fused;
    *composed = s.place_composed;
    return SFHE_OK;
}

int sfhe_select_counts(sfhe_ctx* c, uint64_t* batches, uint64_t* fold_fused, uint64_t* fold_composed) {
    REQUIRE(c && batches && fold_fused && fold_composed, "null argument");
    auto s = c->cc->GetOpStats();
    *batches = s.select_batches;
    *fold_fused = s.fold_fused;
    *fold_composed = s.fold_composed;
    return SFHE_OK;
}

int sfhe_select_cols_counts(sfhe_ctx* c, uint64_t* columns, uint64_t* fused, uint64_t* composed) {
    REQUIRE(c && columns && fused && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *columns = s.select_columns;
    *fused = s.fold_cols_fused;
    *composed = s.fold_cols_composed;
    return SFHE_OK;
}

int sfhe_const_term_counts(sfhe_ctx* c, uint64_t* merged, uint64_t* single, uint64_t* composed) {
    REQUIRE(c && merged && single && composed, "null argument");
    auto s = c->cc->GetOpStats();
    *merged = s.const_merged;
    *single = s.const_single;
    *composed = s.const_composed;
    return SFHE_OK;
}

void sfhe_ct_free(sfhe_ct* ct) { delete ct; }

int sfhe_ct_clone(const sfhe_ct* ct, sfhe_ct** out) {
    REQUIRE(ct && out, "null argument");
    return guard([&] { *out = wrap(ct->ct->Clone()); });
}

int sfhe_ct_info(const sfhe_ct* ct, uint32_t* level, uint32_t* slots, uint32_t* limbs) {
    REQUIRE(ct, "null ciphertext");
    if (level) *level = ct->ct->GetLevel();
    if (slots) *slots = ct->ct->GetSlots();
    if (limbs) *limbs = ct->ct->GetNumLimbs();
    return SFHE_OK;
}

int sfhe_ct_set_slots(sfhe_ct* ct, uint32_t slots) {
    REQUIRE(ct && slots && !(slots & (slots - 1)), "slots must be a power of two");
    ct->ct->SetSlots(slots);
    return SFHE_OK;
}

int sfhe_ct_download(sfhe_ctx* c, const sfhe_ct* ct, uint64_t* out, size_t cap) {
    REQUIRE(c && ct && out, "null argument");
    const size_t n = c->cc->GetRingDimension();
    const size_t L = ct->ct->GetNumLimbs();
    REQUIRE(cap >= 2 * L * n, "output buffer too small");
    return guard([&] { c->cc->DownloadRows(ct->ct, out); });
}

#define BINOP(name, expr)                                                           \
    int name(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, sfhe_ct** out) {       \
        REQUIRE(c && a && b && out, "null argument");                               \
        return guard([&] { *out = wrap(expr); });                                   \
    }
BINOP(sfhe_eval_add, c->cc->EvalAdd(a->ct, b->ct))
BINOP(sfhe_eval_sub, c->cc->EvalSub(a->ct, b->ct))
BINOP(sfhe_eval_mult, c->cc->EvalMult(a->ct, b->ct))

int sfhe_eval_add_const(sfhe_ctx* c, const sfhe_ct* a, double k, sfhe_ct** out) {
    REQUIRE(c && a && out, "null argument");
    return guard([&] { *out = wrap(c->cc->EvalAdd(a->ct, k)); });
}
int sfhe_eval_mult_const(sfhe_ctx* c, const sfhe_ct* a, double k, sfhe_ct** out) {
    REQUIRE(c && a && out, "null argument");
    return guard([&] { *out = wrap(c->cc->EvalMult(a->ct, k)); });
}
int sfhe_eval_mult_plain(sfhe_ctx* c, const sfhe_ct* a, const double* v, size_t len,
                         uint32_t slots, sfhe_ct** out) {
    REQUIRE(c && a && out && (v || !len), "null argument");
    return guard([&] {
        auto pt = c->cc->MakeCKKSPackedPlaintext(std::vector<double>(v, v + len), 1,
                                                 a->ct->GetLevel(), nullptr, slots);
        *out = wrap(c->cc->EvalMult(a->ct, pt));
    });
}
int sfhe_eval_rotate(sfhe_ctx* c, const sfhe_ct* a, int32_t r, sfhe_ct** out) {
    REQUIRE(c && a && out, "null argument");
    return guard([&] { *out = wrap(c->cc->EvalRotate(a->ct, r)); });
}
int sfhe_eval_rotate_sum(sfhe_ctx* c, const sfhe_ct* const* a, const int32_t* r, size_t count, sfhe_ct** out) {
    REQUIRE(c && a && r && out && count, "null argument");
    for (size_t k = 0; k < count; ++k) REQUIRE(a[k], "null argument");
    return guard([&] {
        std::vector<Ciphertext<DCRTPoly>> v;
        for (size_t k = 0; k < count; ++k) v.push_back(a[k]->ct);
        *out = wrap(c->cc->EvalRotateSum(v, std::vector<int32_t>(r, r + count)));
    });
}
int sfhe_eval_rotate_fold(sfhe_ctx* c, const sfhe_ct* a, int32_t stride, uint32_t count, sfhe_ct** out) {
    REQUIRE(c && a && out, "null argument");
    REQUIRE(count >= 2 && count <= 8, "count must be in [2, 8]");
    return guard([&] { *out = wrap(c->cc->EvalRotateFold(a->ct, stride, count)); });
}
int sfhe_eval_rotate_fold_many(sfhe_ctx* c, const sfhe_ct* const* cts, size_t ncts, int32_t stride, uint32_t count,
                               sfhe_ct** outs) {
    REQUIRE(c && cts && outs, "null argument");
    REQUIRE(ncts >= 1, "no ciphertexts");
    for (size_t i = 0; i < ncts; ++i) REQUIRE(cts[i], "null ciphertext");
    REQUIRE(count >= 2 && count <= 8, "count must be in [2, 8]");
    return guard([&] {
        std::vector<Ct> in;
        for (size_t i = 0; i < ncts; ++i) in.push_back(cts[i]->ct);
        auto folded = c->cc->EvalRotateFoldMany(in, stride, count);
        for (size_t i = 0; i < ncts; ++i) outs[i] = wrap(folded[i]);
    });
}
int sfhe_bootstrap_setup(sfhe_ctx* c, uint32_t budget_c2s, uint32_t budget_s2c, uint32_t slots) {
    REQUIRE(c, "null argument");
    REQUIRE(c->keys.secretKey, "sfhe_keygen must be called first");
    return guard([&] {
        c->cc->EvalBootstrapSetup({budget_c2s, budget_s2c}, {0, 0}, slots);
        c->cc->EvalBootstrapKeyGen(c->keys.secretKey, slots);
    });
}
int sfhe_bootstrap_depth(sfhe_ctx* c, uint32_t budget_c2s, uint32_t budget_s2c, uint32_t slots, uint32_t* depth) {
    REQUIRE(c && depth, "null argument");
    return guard([&] { *depth = c->cc->GetBootstrapDepth({budget_c2s, budget_s2c}, slots); });
}
int sfhe_bootstrap(sfhe_ctx* c, const sfhe_ct* a, uint32_t iterations, uint32_t precision, sfhe_ct** out) {
    REQUIRE(c && a && out, "null argument");
    return guard([&] { *out = wrap(c->cc->EvalBootstrap(a->ct, iterations, precision)); });
}
int sfhe_eval_chebyshev(sfhe_ctx* c, const sfhe_ct* x, const double* coeffs, size_t count,
                        double a, double b, sfhe_ct** out) {
    REQUIRE(c && x && coeffs && count && out, "null argument");
    return guard([&] {
        *out = wrap(c->cc->EvalChebyshevSeriesPS(x->ct, std::vector<double>(coeffs, coeffs + count), a, b));
    });
}

int sfhe_sign(sfhe_ctx* c, const sfhe_ct* x, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(c && x && out, "null argument");
    REQUIRE(n == 3 || n == 4, "composite sign degree n must be 3 or 4");
    return guard([&] { *out = wrap(sign(x->ct, c->cc, SignFunc::CompositeSign, cfgOf(n, dg, df))); });
}

int sfhe_compare(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, int n, int dg, int df,
                 sfhe_ct** out) {
    REQUIRE(c && a && b && out, "null argument");
    REQUIRE(n == 3 || n == 4, "composite sign degree n must be 3 or 4");
    return guard([&] {
        Comparison cmp;
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(cmp.compare(c->cc, a->ct, b->ct, SignFunc::CompositeSign, cfg));
    });
}

int sfhe_direct_sort_params(uint32_t N, uint32_t* depth, int32_t* rot, size_t cap, size_t* count) {
    const sfhe::SizeParams* p = sfhe::sizeParams((int)N);
    REQUIRE(p, "N has no DirectSort size parameters (reference table: 4 .. 2048)");
    return guard([&] {
        const auto& r = p->rotations;
        if (depth) *depth = (uint32_t)p->multDepth;
        if (count) *count = r.size();
        for (size_t i = 0; i < r.size() && i < cap && rot; ++i) rot[i] = r[i];
    });
}

int sfhe_select_params(uint32_t N, uint32_t* depth, int32_t* rot, size_t cap, size_t* count) {
    const sfhe::SizeParams* p = sfhe::sizeParams((int)N);
    REQUIRE(p && validN(N), "N has no selection parameters (a power of two in [4, 1024])");
    return guard([&] {
        // the sort's keys united with the radix-4 fold amounts {s, 2s, 3s : s = 4^i < N}
        std::set<int> r(p->rotations.begin(), p->rotations.end());
        for (int s = 1; s < (int)N; s *= 4)
            for (int k = 1; k <= 3; ++k) r.insert(k * s);
        if (depth) *depth = (uint32_t)p->multDepth;
        if (count) *count = r.size();
        size_t i = 0;
        for (int v : r) {
            if (i >= cap || !rot) break;
            rot[i++] = v;
        }
    });
}

int sfhe_doubled_sinc_coeffs(uint32_t N, double* out, size_t cap, size_t* count) {
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    return guard([&] {
        const auto& v = sfhe::doubledSincCoefficients((int)N);
        if (count) *count = v.size();
        for (size_t i = 0; i < v.size() && i < cap && out; ++i) out[i] = v[i];
    });
}

int sfhe_sorter_create(sfhe_ctx* c, uint32_t N, int debug, sfhe_sorter** out) {
    return sfhe_sorter_create_rot(c, N, debug, nullptr, 0, out);
}

int sfhe_sorter_create_rot(sfhe_ctx* c, uint32_t N, int debug, const int32_t* rotations, size_t nrot,
                           sfhe_sorter** out) {
    REQUIRE(c && out, "null argument");
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    REQUIRE(c->keys.publicKey, "sfhe_keygen must be called first");
    REQUIRE(!nrot || rotations, "null rotation list");
    return guard([&] {
        std::shared_ptr<Encryption> enc =
            debug ? std::shared_ptr<Encryption>(std::make_shared<DebugEncryption>(c->cc, c->keys))
                  : std::make_shared<Encryption>(c->cc, c->keys.publicKey);
        const auto rot = rotations ? std::vector<int>(rotations, rotations + nrot)
                                   : sfhe::sizeParams((int)N)->rotations;
        auto s = std::make_unique<sfhe_sorter>();
        s->ctx = c;
        switch (N) {
#define CASE(K) \
    case K: s->impl.reset(new Sorter<K>(c->cc, c->keys.publicKey, rot, enc)); break;
            CASE(4) CASE(8) CASE(16) CASE(32) CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
        }
        *out = s.release();
    });
}

void sfhe_sorter_destroy(sfhe_sorter* s) { delete s; }

int sfhe_sorter_sort(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->sort(in->ct, cfg));
    });
}

int sfhe_sorter_rank(sfhe_sorter* s, const sfhe_ct* in, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->rank(in->ct, cfg));
    });
}

int sfhe_sorter_sort_stable(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->sortStable(in->ct, cfg));
    });
}

int sfhe_sorter_rank_stable(sfhe_sorter* s, const sfhe_ct* in, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->rankStable(in->ct, cfg));
    });
}

int sfhe_sorter_place(sfhe_sorter* s, const sfhe_ct* rank, sfhe_ct* in, sfhe_ct** out) {
    REQUIRE(s && rank && in && out, "null argument");
    return guard([&] { *out = wrap(s->impl->place(rank->ct, in->ct)); });
}

int sfhe_sorter_place_many(sfhe_sorter* s, const sfhe_ct* rank, sfhe_ct* const* cols, size_t count, sfhe_ct** outs) {
    REQUIRE(s && rank && cols && outs, "null argument");
    REQUIRE(count >= 1 && count <= SFHE_MAX_COLUMNS, "column count out of range (1 .. SFHE_MAX_COLUMNS)");
    for (size_t i = 0; i < count; ++i) REQUIRE(cols[i], "null column");
    return guard([&] {
        std::vector<Ct> in;
        for (size_t i = 0; i < count; ++i) in.push_back(cols[i]->ct);
        auto placed = s->impl->placeMany(rank->ct, in);
        for (size_t i = 0; i < count; ++i) outs[i] = wrap(placed[i]);
    });
}

int sfhe_sorter_sort_records(sfhe_sorter* s, sfhe_ct* keys, sfhe_ct* const* cols, size_t count, int stable, int n,
                             int dg, int df, sfhe_ct** keys_out, sfhe_ct** outs) {
    REQUIRE(s && keys && keys_out && (count == 0 || (cols && outs)), "null argument");
    REQUIRE(count <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    for (size_t i = 0; i < count; ++i) REQUIRE(cols[i], "null column");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> in;
        for (size_t i = 0; i < count; ++i) in.push_back(cols[i]->ct);
        auto sorted = s->impl->sortRecords(keys->ct, in, cfg, stable != 0);
        *keys_out = wrap(sorted[0]);
        for (size_t i = 0; i < count; ++i) outs[i] = wrap(sorted[i + 1]);
    });
}

static int selectTargets(const sfhe_sorter* s, const uint32_t* targets, size_t count, uint32_t N,
                         std::vector<int>* out) {
    (void)s;
    REQUIRE(count >= 1 && count <= N, "target count out of range (1 .. N)");
    std::vector<char> seen(N, 0);
    for (size_t i = 0; i < count; ++i) {
        REQUIRE(targets[i] < N, "target rank out of range (0 .. N - 1)");
        REQUIRE(!seen[targets[i]], "duplicate target rank");
        seen[targets[i]] = 1;
        out->push_back((int)targets[i]);
    }
    return SFHE_OK;
}

int sfhe_sorter_select_ranked(sfhe_sorter* s, const sfhe_ct* rank, const sfhe_ct* in, const uint32_t* targets,
                              size_t count, sfhe_ct** out) {
    REQUIRE(s && rank && in && targets && out, "null argument");
    std::vector<int> t;
    if (int rc = selectTargets(s, targets, count, s->impl->size(), &t)) return rc;
    return guard([&] { *out = wrap(s->impl->selectRanks(rank->ct, in->ct, t)); });
}

int sfhe_sorter_select(sfhe_sorter* s, const sfhe_ct* in, const uint32_t* targets, size_t count, int stable, int n,
                       int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && targets && out, "null argument");
    std::vector<int> t;
    if (int rc = selectTargets(s, targets, count, s->impl->size(), &t)) return rc;
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->select(in->ct, t, cfg, stable != 0));
    });
}

int sfhe_sorter_select_many(sfhe_sorter* s, const sfhe_ct* rank, const sfhe_ct* const* cols, size_t ncols,
                            const uint32_t* targets, size_t count, sfhe_ct** outs) {
    REQUIRE(s && rank && cols && targets && outs, "null argument");
    REQUIRE(ncols >= 1 && ncols <= SFHE_MAX_COLUMNS, "column count out of range (1 .. SFHE_MAX_COLUMNS)");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols[i], "null column");
    std::vector<int> t;
    if (int rc = selectTargets(s, targets, count, s->impl->size(), &t)) return rc;
    return guard([&] {
        std::vector<Ct> in;
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols[i]->ct);
        auto got = s->impl->selectRanksMany(rank->ct, in, t);
        for (size_t i = 0; i < ncols; ++i) outs[i] = wrap(got[i]);
    });
}

int sfhe_sorter_select_records(sfhe_sorter* s, const sfhe_ct* keys, const sfhe_ct* const* cols, size_t ncols,
                               const uint32_t* targets, size_t count, int stable, int n, int dg, int df,
                               sfhe_ct** keys_out, sfhe_ct** outs) {
    REQUIRE(s && keys && targets && keys_out && (ncols == 0 || (cols && outs)), "null argument");
    REQUIRE(ncols <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols[i], "null column");
    std::vector<int> t;
    if (int rc = selectTargets(s, targets, count, s->impl->size(), &t)) return rc;
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> in;
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols[i]->ct);
        auto got = s->impl->selectRecords(keys->ct, in, t, cfg, stable != 0);
        *keys_out = wrap(got[0]);
        for (size_t i = 0; i < ncols; ++i) outs[i] = wrap(got[i + 1]);
    });
}

// the key columns and their direction flags of a lexicographic call
static int lexKeys(const sfhe_ct* const* keys, size_t nkeys, const int* descending, size_t ncols,
                   std::vector<Ct>* out, std::vector<bool>* desc) {
    REQUIRE(nkeys >= 1 && nkeys <= SFHE_LEX_KEYS, "key count out of range (1 .. SFHE_LEX_KEYS)");
    REQUIRE(nkeys + ncols <= 1 + SFHE_MAX_COLUMNS,
            "too many columns (keys and payload columns together: at most 1 + SFHE_MAX_COLUMNS)");
    for (size_t i = 0; i < nkeys; ++i) {
        REQUIRE(keys[i], "null key column");
        out->push_back(keys[i]->ct);
        desc->push_back(descending && descending[i] != 0);
    }
    return SFHE_OK;
}

int sfhe_lex_sort_depth(uint32_t N, int n, int dg, int df, uint32_t nkeys, uint32_t* mult_depth) {
    REQUIRE(mult_depth, "null argument");
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    REQUIRE(nkeys >= 1 && nkeys <= SFHE_LEX_KEYS, "key count out of range (1 .. SFHE_LEX_KEYS)");
    return guard([&] { *mult_depth = (uint32_t)sfhe::lexSortDepth((int)N, CompositeSignConfig(n, dg, df), (int)nkeys); });
}

int sfhe_sorter_rank_lex(sfhe_sorter* s, const sfhe_ct* const* keys, size_t nkeys, const int* descending, int n,
                         int dg, int df, sfhe_ct** out) {
    REQUIRE(s && keys && out, "null argument");
    std::vector<Ct> k;
    std::vector<bool> d;
    if (int rc = lexKeys(keys, nkeys, descending, 0, &k, &d)) return rc;
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->rankLex(k, d, cfg));
    });
}

int sfhe_sorter_sort_records_lex(sfhe_sorter* s, sfhe_ct* const* keys, size_t nkeys, const int* descending,
                                 sfhe_ct* const* cols, size_t ncols, int n, int dg, int df, sfhe_ct** keys_out,
                                 sfhe_ct** outs) {
    REQUIRE(s && keys && keys_out && (ncols == 0 || (cols && outs)), "null argument");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols[i], "null column");
    std::vector<Ct> k;
    std::vector<bool> d;
    if (int rc = lexKeys(keys, nkeys, descending, ncols, &k, &d)) return rc;
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> in;
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols[i]->ct);
        auto sorted = s->impl->sortRecordsLex(k, in, d, cfg);
        for (size_t i = 0; i < nkeys; ++i) keys_out[i] = wrap(sorted[i]);
        for (size_t i = 0; i < ncols; ++i) outs[i] = wrap(sorted[nkeys + i]);
    });
}

int sfhe_sorter_select_records_lex(sfhe_sorter* s, const sfhe_ct* const* keys, size_t nkeys, const int* descending,
                                   const sfhe_ct* const* cols, size_t ncols, const uint32_t* targets, size_t count,
                                   int n, int dg, int df, sfhe_ct** keys_out, sfhe_ct** outs) {
    REQUIRE(s && keys && targets && keys_out && (ncols == 0 || (cols && outs)), "null argument");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols[i], "null column");
    std::vector<Ct> k;
    std::vector<bool> d;
    if (int rc = lexKeys(keys, nkeys, descending, ncols, &k, &d)) return rc;
    std::vector<int> t;
    if (int rc = selectTargets(s, targets, count, s->impl->size(), &t)) return rc;
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> in;
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols[i]->ct);
        auto got = s->impl->selectRecordsLex(k, in, t, d, cfg);
        for (size_t i = 0; i < nkeys; ++i) keys_out[i] = wrap(got[i]);
        for (size_t i = 0; i < ncols; ++i) outs[i] = wrap(got[nkeys + i]);
    });
}

int sfhe_eval_lex_step(sfhe_ctx* c, const sfhe_ct* v, const sfhe_ct* q, const sfhe_ct* u, sfhe_ct** out) {
    REQUIRE(c && v && q && u && out, "null argument");
    return guard([&] { *out = wrap(c->cc->EvalLexStep(v->ct, q->ct, u->ct)); });
}

int sfhe_eval_mult_sum2(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, const sfhe_ct* a2, const sfhe_ct* b2,
                        const sfhe_ct* r, sfhe_ct** out) {
    REQUIRE(c && a && b && a2 && b2 && out, "null argument");
    return guard([&] {
        for (const sfhe_ct* x : {a, b, a2, b2, r})
            if (x) c->cc->Settle(x->ct);
        *out = wrap(c->cc->EvalMultSum2(a->ct, b->ct, a2->ct, b2->ct, r ? r->ct : nullptr));
    });
}

int sfhe_eval_mult_sum(sfhe_ctx* c, const sfhe_ct* const* a, const sfhe_ct* const* b, size_t n, const sfhe_ct* r,
                       sfhe_ct** out) {
    REQUIRE(c && a && b && out, "null argument");
    REQUIRE(n >= 1, "no terms");
    for (size_t i = 0; i < n; ++i) REQUIRE(a[i] && b[i], "null term");
    return guard([&] {
        std::vector<lbcrypto::CryptoContextImpl<lbcrypto::DCRTPoly>::MultTerm> terms;
        for (size_t i = 0; i < n; ++i) {
            c->cc->Settle(a[i]->ct);
            c->cc->Settle(b[i]->ct);
            terms.emplace_back(a[i]->ct, b[i]->ct);
        }
        lbcrypto::CryptoContextImpl<lbcrypto::DCRTPoly>::MultAddend add;
        if (r) {
            c->cc->Settle(r->ct);
            add.r = r->ct;
        }
        *out = wrap(c->cc->EvalMultSum(terms, add));
    });
}

int sfhe_eval_mult_sum_many(sfhe_ctx* c, const sfhe_ct* const* a, const sfhe_ct* const* b, const size_t* counts,
                            size_t nops, const sfhe_ct* const* r, sfhe_ct** out) {
    REQUIRE(c && a && b && counts && out, "null argument");
    size_t total = 0;
    for (size_t o = 0; o < nops; ++o) {
        REQUIRE(counts[o] >= 1, "an op without terms");
        total += counts[o];
    }
    for (size_t i = 0; i < total; ++i) REQUIRE(a[i] && b[i], "null term");
    return guard([&] {
        using CC = lbcrypto::CryptoContextImpl<lbcrypto::DCRTPoly>;
        std::vector<CC::MultSumOp> ops(nops);
        size_t at = 0;
        for (size_t o = 0; o < nops; ++o) {
            for (size_t k = 0; k < counts[o]; ++k, ++at) {
                c->cc->Settle(a[at]->ct);
                c->cc->Settle(b[at]->ct);
                ops[o].terms.emplace_back(a[at]->ct, b[at]->ct);
            }
            if (r && r[o]) {
                c->cc->Settle(r[o]->ct);
                ops[o].add.r = r[o]->ct;
            }
        }
        auto res = c->cc->EvalMultSumMany(ops);
        for (size_t o = 0; o < nops; ++o) out[o] = wrap(res[o]);
    });
}

int sfhe_ct_relabel_scale(const sfhe_ct* ct, double factor, sfhe_ct** out) {
    REQUIRE(ct && out, "null argument");
    return guard([&] {
        auto x = ct->ct->Clone();
        x->scale *= factor;
        *out = wrap(x);
    });
}

static_assert(SFHE_MAX_COLUMNS == CryptoContextImpl<DCRTPoly>::kGateMaxColumns,
              "EvalGateSumMany's column limit is the record entry points'");

int sfhe_group_params(uint32_t N, uint32_t* mult_depth, int32_t* rot, size_t cap, size_t* count) {
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    return guard([&] {
        // the rank's amounts in the layout of the size table's ring (2^17): baby
        // steps, giant steps, the batches' offsets and the partition folds.  A
        // smaller ring uses a subset of them or composes its own from them.
        const sfhe::RankLayout L((int)N, 1 << 16);
        std::set<int> r;
        for (int i = 1; i < L.npRank; ++i) r.insert(i);
        for (int j = 1; j < L.P / L.npRank; ++j) r.insert(j * L.npRank);
        for (int b = 1; b < L.B; ++b) r.insert(b * L.P);
        for (int sft = L.S / 2; sft >= (int)N; sft /= 2) r.insert(sft);
        if (mult_depth) *mult_depth = (uint32_t)sfhe::groupDepth(sfhe::defaultSignConfig((int)N));
        if (count) *count = r.size();
        size_t i = 0;
        for (int v : r) {
            if (i >= cap || !rot) break;
            rot[i++] = v;
        }
    });
}

int sfhe_sorter_group(sfhe_sorter* s, const sfhe_ct* keys, const sfhe_ct* const* cols, size_t ncols, int want_index,
                      int n, int dg, int df, sfhe_ct** count, sfhe_ct** index, sfhe_ct** sums_out) {
    REQUIRE(s && keys && count && (!want_index || index) && (ncols == 0 || (cols && sums_out)), "null argument");
    REQUIRE(ncols <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols[i], "null column");
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> in;
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols[i]->ct);
        auto got = s->impl->group(keys->ct, in, cfg, want_index != 0);
        *count = wrap(got[0]);
        if (index) *index = want_index ? wrap(got[1]) : nullptr;
        for (size_t i = 0; i < ncols; ++i) sums_out[i] = wrap(got[2 + i]);
    });
}

int sfhe_eval_gate_sum_many(sfhe_ctx* c, const sfhe_ct* const* q, size_t nq, const sfhe_ct* const* u, size_t ncols,
                            sfhe_ct** outs) {
    REQUIRE(c && q && (ncols == 0 || (u && outs)), "null argument");
    REQUIRE(nq >= 1, "no gates");
    REQUIRE(ncols <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    for (size_t b = 0; b < nq; ++b) {
        REQUIRE(q[b], "null gate");
        REQUIRE(q[b]->ct->GetLevel() == q[0]->ct->GetLevel(), "the gates must be at one level");
    }
    for (size_t i = 0; i < ncols * nq; ++i) {
        REQUIRE(u[i], "null operand");
        REQUIRE(u[i]->ct->GetLevel() <= q[0]->ct->GetLevel(),
                "the operands must have at least the gates' limbs (a level not above the gates')");
    }
    return guard([&] {
        std::vector<Ct> qs;
        for (size_t b = 0; b < nq; ++b) qs.push_back(q[b]->ct);
        std::vector<std::vector<Ct>> us(ncols);
        for (size_t k = 0; k < ncols; ++k)
            for (size_t b = 0; b < nq; ++b) us[k].push_back(u[k * nq + b]->ct);
        auto got = c->cc->EvalGateSumMany(qs, us);
        for (size_t k = 0; k < ncols; ++k) outs[k] = wrap(got[k]);
    });
}

// the rank's amounts in the layout of the size table's ring (2^17): baby steps,
// giant steps, the batches' offsets and the partition folds.  A smaller ring
// uses a subset of them or composes its own from them.
static std::set<int> rankRotations(uint32_t N) {
    const sfhe::RankLayout L((int)N, 1 << 16);
    std::set<int> r;
    for (int i = 1; i < L.npRank; ++i) r.insert(i);
    for (int j = 1; j < L.P / L.npRank; ++j) r.insert(j * L.npRank);
    for (int b = 1; b < L.B; ++b) r.insert(b * L.P);
    for (int sft = L.S / 2; sft >= (int)N; sft /= 2) r.insert(sft);
    return r;
}

int sfhe_window_params(uint32_t N, uint32_t* mult_depth, int32_t* rot, size_t cap, size_t* count) {
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    return guard([&] {
        const std::set<int> r = rankRotations(N);
        if (mult_depth) *mult_depth = (uint32_t)sfhe::windowDepth(sfhe::defaultSignConfig((int)N));
        if (count) *count = r.size();
        size_t i = 0;
        for (int v : r) {
            if (i >= cap || !rot) break;
            rot[i++] = v;
        }
    });
}

int sfhe_sorter_window(sfhe_sorter* s, const sfhe_ct* keys, const sfhe_ct* const* cols, size_t ncols, int frame,
                       int want_count, int n, int dg, int df, sfhe_ct** count, sfhe_ct** sums_out) {
    REQUIRE(s && keys && (!want_count || count) && (ncols == 0 || (cols && sums_out)), "null argument");
    REQUIRE(ncols <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    REQUIRE(frame >= SFHE_FRAME_ROWS && frame <= SFHE_FRAME_BELOW, "unknown frame (0 rows, 1 range, 2 below)");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols[i], "null column");
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> in;
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols[i]->ct);
        auto got = s->impl->window(keys->ct, in, cfg, frame, want_count != 0);
        if (count) *count = want_count ? wrap(got[0]) : nullptr;
        for (size_t i = 0; i < ncols; ++i) sums_out[i] = wrap(got[1 + i]);
    });
}

int sfhe_eval_weight_sum_many(sfhe_ctx* c, const sfhe_ct* const* v, size_t nv, const double* const* weights,
                              size_t len, uint32_t slots, const sfhe_ct* const* u, size_t ncols, sfhe_ct** outs) {
    REQUIRE(c && v && weights && (ncols == 0 || (u && outs)), "null argument");
    REQUIRE(nv >= 1, "no gates");
    REQUIRE(ncols <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    for (size_t b = 0; b < nv; ++b) {
        REQUIRE(v[b], "null gate");
        REQUIRE(weights[b] || !len, "null weight vector");
        REQUIRE(v[b]->ct->GetLevel() == v[0]->ct->GetLevel(), "the gates must be at one level");
    }
    for (size_t i = 0; i < ncols * nv; ++i) {
        REQUIRE(u[i], "null operand");
        REQUIRE(u[i]->ct->GetLevel() <= v[0]->ct->GetLevel(),
                "the operands must have at least the gates' limbs (a level not above the gates')");
    }
    return guard([&] {
        std::vector<Ct> vs;
        std::vector<Plaintext> ps;
        for (size_t b = 0; b < nv; ++b) {
            vs.push_back(v[b]->ct);
            ps.push_back(c->cc->MakeCKKSPackedPlaintext(std::vector<double>(weights[b], weights[b] + len), 1,
                                                        v[0]->ct->GetLevel(), nullptr, slots));
        }
        std::vector<std::vector<Ct>> us(ncols);
        for (size_t k = 0; k < ncols; ++k)
            for (size_t b = 0; b < nv; ++b) us[k].push_back(u[k * nv + b]->ct);
        auto got = c->cc->EvalWeightSumMany(vs, ps, us);
        for (size_t k = 0; k < ncols; ++k) outs[k] = wrap(got[k]);
    });
}

int sfhe_join_params(uint32_t N, uint32_t nkeys, uint32_t* mult_depth, int32_t* rot, size_t cap, size_t* count) {
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    REQUIRE(nkeys >= 1 && nkeys <= SFHE_LEX_KEYS, "key count out of range (1 .. 4)");
    return guard([&] {
        const std::set<int> r = rankRotations(N);
        if (mult_depth) *mult_depth = (uint32_t)sfhe::joinDepth(sfhe::defaultSignConfig((int)N), (int)nkeys);
        if (count) *count = r.size();
        size_t i = 0;
        for (int v : r) {
            if (i >= cap || !rot) break;
            rot[i++] = v;
        }
    });
}

int sfhe_sorter_join(sfhe_sorter* s, const sfhe_ct* const* keys_a, const sfhe_ct* const* keys_b, size_t nkeys,
                     const sfhe_ct* const* cols_b, size_t ncols, int n, int dg, int df, sfhe_ct** count,
                     sfhe_ct** sums_out) {
    REQUIRE(s && keys_a && keys_b && count && (ncols == 0 || (cols_b && sums_out)), "null argument");
    REQUIRE(nkeys >= 1 && nkeys <= SFHE_LEX_KEYS, "key count out of range (1 .. 4)");
    REQUIRE(ncols <= SFHE_MAX_COLUMNS, "column count out of range (0 .. SFHE_MAX_COLUMNS)");
    for (size_t k = 0; k < nkeys; ++k) REQUIRE(keys_a[k] && keys_b[k], "null key");
    for (size_t i = 0; i < ncols; ++i) REQUIRE(cols_b[i], "null column");
    return guard([&] {
        auto cfg = cfgOf(n, dg, df);
        std::vector<Ct> ka, kb, in;
        for (size_t k = 0; k < nkeys; ++k) {
            ka.push_back(keys_a[k]->ct);
            kb.push_back(keys_b[k]->ct);
        }
        for (size_t i = 0; i < ncols; ++i) in.push_back(cols_b[i]->ct);
        auto got = s->impl->join(ka, kb, in, cfg);
        *count = wrap(got[0]);
        for (size_t i = 0; i < ncols; ++i) sums_out[i] = wrap(got[1 + i]);
    });
}

int sfhe_eval_gate_or(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, sfhe_ct** out) {
    REQUIRE(c && a && b && out, "null argument");
    REQUIRE(a->ct->GetSlots() == b->ct->GetSlots(), "the operands must have one slot count");
    return guard([&] { *out = wrap(c->cc->EvalGateOr(a->ct, b->ct)); });
}

int sfhe_sorter_sort_hybrid1(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    REQUIRE(s->ctx->keys.secretKey, "sfhe_keygen must be called first");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->hybrid1(in->ct, cfg, s->ctx->keys.secretKey));
    });
}

int sfhe_sorter_sort_hybrid(sfhe_sorter* s, sfhe_ct* in, int variant, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    REQUIRE(variant == 0 || variant == 2, "variant must be 0 (sort_hybrid) or 2 (sort_hybrid2)");
    REQUIRE(s->ctx->keys.secretKey, "sfhe_keygen must be called first");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->hybrid(in->ct, cfg, s->ctx->keys.secretKey, variant));
    });
}

int sfhe_sorter_place_2n(sfhe_sorter* s, const sfhe_ct* rank, sfhe_ct* in, sfhe_ct** out) {
    REQUIRE(s && rank && in && out, "null argument");
    return guard([&] { *out = wrap(s->impl->place2N(rank->ct, in->ct)); });
}

int sfhe_sorter_sort_bitonic(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    REQUIRE(n == 3 || n == 4, "composite sign degree n must be 3 or 4");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        auto cfg = cfgOf(n, dg, df);
        *out = wrap(s->impl->bitonic(in->ct, cfg));
    });
}

int sfhe_save(sfhe_ctx* c, const char* dir) {
    REQUIRE(c && dir, "null argument");
    return guard([&] {
        const std::string d(dir);
        auto put = [&](const std::string& name, auto&& write) {
            std::ofstream f(d + "/" + name, std::ios::binary | std::ios::trunc);
            if (!f.is_open() || !write(f) || !f.good()) throw std::invalid_argument("cannot write " + d + "/" + name);
        };
        put("cc.bin", [&](std::ostream& f) { return Serial::Serialize(c->cc, f, SerType::BINARY); });
        put("pub.bin", [&](std::ostream& f) { return Serial::Serialize(c->keys.publicKey, f, SerType::BINARY); });
        if (c->keys.secretKey)
            put("sk.bin", [&](std::ostream& f) { return Serial::Serialize(c->keys.secretKey, f, SerType::BINARY); });
        // this context's key pair only (other engines in the process keep theirs)
        const std::string tag = KeyTagString(c->cc->KeyTag());
        put("mult.bin", [&](std::ostream& f) {
            return CryptoContextImpl<DCRTPoly>::SerializeEvalMultKey(f, SerType::BINARY, tag);
        });
        put("rot.bin", [&](std::ostream& f) {
            return CryptoContextImpl<DCRTPoly>::SerializeEvalAutomorphismKey(f, SerType::BINARY, tag);
        });
    });
}

int sfhe_load(const char* dir, sfhe_ctx** out) {
    REQUIRE(dir && out, "null argument");
    return guard([&] {
        const std::string d(dir);
        auto get = [&](const std::string& name, bool required, auto&& read) {
            std::ifstream f(d + "/" + name, std::ios::binary);
            if (!f.is_open()) {
                if (required) throw std::invalid_argument("cannot open " + d + "/" + name);
                return;
            }
            if (!read(f)) throw std::invalid_argument("cannot deserialize " + d + "/" + name);
        };
        auto ctx = std::make_unique<sfhe_ctx>();
        get("cc.bin", true, [&](std::istream& f) { return Serial::Deserialize(ctx->cc, f, SerType::BINARY); });
        get("pub.bin", true, [&](std::istream& f) { return Serial::Deserialize(ctx->keys.publicKey, f, SerType::BINARY); });
        get("sk.bin", false, [&](std::istream& f) { return Serial::Deserialize(ctx->keys.secretKey, f, SerType::BINARY); });
        get("mult.bin", true, [&](std::istream& f) { return CryptoContextImpl<DCRTPoly>::DeserializeEvalMultKey(f, SerType::BINARY); });
        get("rot.bin", true, [&](std::istream& f) {
            return CryptoContextImpl<DCRTPoly>::DeserializeEvalAutomorphismKey(f, SerType::BINARY);
        });
        *out = ctx.release();
    });
}

int sfhe_ct_save(sfhe_ctx* c, const sfhe_ct* ct, const char* path) {
    REQUIRE(c && ct && path, "null argument");
    return guard([&] {
        if (!Serial::SerializeToFile(std::string(path), ct->ct, SerType::BINARY))
            throw std::invalid_argument(std::string("cannot write ") + path);
    });
}

int sfhe_ct_load(sfhe_ctx* c, const char* path, sfhe_ct** out) {
    REQUIRE(c && path && out, "null argument");
    return guard([&] {
        Ct ct;
        if (!Serial::DeserializeFromFile(std::string(path), ct, SerType::BINARY))
            throw std::invalid_argument(std::string("cannot read ") + path);
        *out = wrap(ct);
    });
}

int sfhe_kway_sort(sfhe_ctx* c, const sfhe_ct* in, int k, int M, int n, int dg, int df, uint32_t mult_depth,
                   sfhe_ct** out) {
    REQUIRE(c && in && out, "null argument");
    REQUIRE(k == 2 || k == 3 || k == 5, "k must be 2, 3 or 5");
    REQUIRE(M >= 1 && M <= 16, "M out of range");
    REQUIRE(n == 3 || n == 4, "composite sign degree n must be 3 or 4");
    long len = 1;
    for (int i = 0; i < M; ++i) len *= k;
    REQUIRE(len <= (long)in->ct->GetSlots(), "k^M exceeds the ciphertext's slots");
    return guard([&] {
        Quiet q(c->quiet);
        // (the sorter keeps the keys only for its debug decryptions)
        kwaySort::Sorter sorter(c->cc, nullptr, (long)in->ct->GetSlots(), k, M, c->keys.secretKey,
                                c->keys.publicKey);
        SignConfig cfg(CompositeSignConfig(n, dg, df), (int)mult_depth);
        Ct x = in->ct->Clone(), y;
        sorter.sorter(x, y, cfg);
        if (!y) throw OpenFHEException("k-way sorter: no stage schedule for this k");
        *out = wrap(y);
    });
}

}  // extern "C"

namespace {
struct KWayBase {
    virtual ~KWayBase() = default;
    virtual Ct run(const Ct& in, SignConfig& cfg) = 0;
    virtual size_t graphNodes() const = 0;
    virtual bool graphFamilyTime(uint32_t family, int reps, double* ms, uint64_t* launches, double* bytes) = 0;
};
template <int N>
struct KWayImpl : KWayBase {
    KWayAdapter<N> a;
    KWayImpl(sfhe_ctx* c, int k, int M)
        : a(c->cc, c->keys.publicKey, c->keys.secretKey,
            std::make_shared<Encryption>(c->cc, c->keys.publicKey), k, M) {}
    Ct run(const Ct& in, SignConfig& cfg) override { return a.sort(in, SignFunc::CompositeSign, cfg); }
    size_t graphNodes() const override { return a.graphNodes(); }
    bool graphFamilyTime(uint32_t family, int reps, double* ms, uint64_t* launches, double* bytes) override {
        return a.graphFamilyTime(family, reps, ms, launches, bytes);
    }
};
std::unique_ptr<KWayBase> makeKWay(sfhe_ctx* c, uint32_t N, int k, int M) {
    switch (N) {
#define SFHE_KWAY_N(v) \
    case v: return std::make_unique<KWayImpl<v>>(c, k, M);
        SFHE_KWAY_N(4) SFHE_KWAY_N(8) SFHE_KWAY_N(16) SFHE_KWAY_N(32) SFHE_KWAY_N(64) SFHE_KWAY_N(128)
        SFHE_KWAY_N(256) SFHE_KWAY_N(512) SFHE_KWAY_N(1024) SFHE_KWAY_N(9) SFHE_KWAY_N(27) SFHE_KWAY_N(81)
        SFHE_KWAY_N(243) SFHE_KWAY_N(729) SFHE_KWAY_N(25) SFHE_KWAY_N(125) SFHE_KWAY_N(625)
#undef SFHE_KWAY_N
    }
    return nullptr;
}
}  // namespace

struct sfhe_kway {
    sfhe_ctx* ctx;
    std::unique_ptr<KWayBase> impl;
};

extern "C" {

int sfhe_kway_create(sfhe_ctx* c, uint32_t N, int k, int M, sfhe_kway** out) {
    REQUIRE(c && out, "null argument");
    REQUIRE(k == 2 || k == 3 || k == 5, "k must be 2, 3 or 5");
    long len = 1;
    for (int i = 0; i < M && len <= (1 << 20); ++i) len *= k;
    REQUIRE(M >= 1 && len == (long)N, "N must equal k^M");
    return guard([&] {
        auto impl = makeKWay(c, N, k, M);
        if (!impl) throw std::invalid_argument("unsupported N for the k-way network");
        *out = new sfhe_kway{c, std::move(impl)};
    });
}

int sfhe_kway_run(sfhe_kway* s, const sfhe_ct* in, int n, int dg, int df, uint32_t mult_depth, sfhe_ct** out) {
    REQUIRE(s && in && out, "null argument");
    REQUIRE(n == 3 || n == 4, "composite sign degree n must be 3 or 4");
    return guard([&] {
        Quiet q(s->ctx->quiet);
        SignConfig cfg(CompositeSignConfig(n, dg, df), (int)mult_depth);
        *out = wrap(s->impl->run(in->ct, cfg));
    });
}

void sfhe_kway_destroy(sfhe_kway* s) { delete s; }

int sfhe_kway_graph_family_time(sfhe_kway* s, uint32_t family, int reps, double* ms, uint64_t* launches,
                                double* bytes) {
    REQUIRE(s && ms && reps > 0, "null argument");
    REQUIRE(family <= SFHE_KFAM_ALL, "unknown kernel family");
    return guard([&] {
        if (!s->impl->graphFamilyTime(family, reps, ms, launches, bytes))
            throw std::runtime_error("no captured k-way graph with kernels of that family");
    });
}

int sfhe_kway_graph_nodes(const sfhe_kway* s, uint64_t* nodes) {
    REQUIRE(s && nodes, "null argument");
    *nodes = s->impl->graphNodes();
    return SFHE_OK;
}

int sfhe_kway_params(uint32_t N, uint32_t* batch, uint32_t* mult_depth, uint32_t* budget_c2s, uint32_t* budget_s2c,
                     int32_t* rotations, size_t cap, size_t* count) {
    REQUIRE(N >= 2 && N <= (1u << 16), "N out of range");
    uint32_t b = 1;
    while (b < N) b <<= 1;
    if (batch) *batch = b;
    if (mult_depth) *mult_depth = 40;
    if (budget_c2s) *budget_c2s = N <= 128 ? 4 : 5;
    if (budget_s2c) *budget_s2c = N <= 128 ? 4 : 5;
    std::vector<int32_t> r;
    for (uint32_t i = 1; i < N; i *= 2) {
        r.push_back((int32_t)i);
        r.push_back(-(int32_t)i);
    }
    if (count) *count = r.size();
    for (size_t i = 0; i < r.size() && i < cap && rotations; ++i) rotations[i] = r[i];
    return SFHE_OK;
}

int sfhe_hybrid1_params(uint32_t N, uint32_t* mult_depth, int32_t* rotations, size_t cap, size_t* count) {
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    const sfhe::SizeParams* p = sfhe::hybrid1Params((int)N);
    if (mult_depth) *mult_depth = (uint32_t)p->multDepth;
    if (count) *count = p->rotations.size();
    for (size_t i = 0; i < p->rotations.size() && i < cap && rotations; ++i) rotations[i] = p->rotations[i];
    return SFHE_OK;
}

int sfhe_hybrid_params(uint32_t N, int variant, uint32_t* mult_depth, int32_t* rotations, size_t cap,
                       size_t* count) {
    REQUIRE(validN(N), "N must be a power of two in [4, 1024]");
    REQUIRE(variant == 0 || variant == 2, "variant must be 0 (sort_hybrid) or 2 (sort_hybrid2)");
    const sfhe::SizeParams* p = sfhe::hybridParams((int)N, variant);
    if (mult_depth) *mult_depth = (uint32_t)p->multDepth;
    if (count) *count = p->rotations.size();
    for (size_t i = 0; i < p->rotations.size() && i < cap && rotations; ++i) rotations[i] = p->rotations[i];
    return SFHE_OK;
}

int sfhe_sorter_graph_family_time(sfhe_sorter* s, uint32_t family, int reps, double* ms, uint64_t* launches,
                                  double* bytes) {
    REQUIRE(s && ms && reps > 0, "null argument");
    static_assert(SFHE_KFAM_OTHER == SFP_FAM_COUNT && SFHE_KFAM_ALL == SFP_FAM_ALL, "family numbering");
    REQUIRE(family <= SFHE_KFAM_ALL, "unknown kernel family");
    return guard([&] {
        if (!s->impl->graphFamilyTime(family, reps, ms, launches, bytes))
            throw std::runtime_error("no captured sort graph (or no graphs on this backend)");
    });
}

int sfhe_sorter_graph_ntt_time(sfhe_sorter* s, int reps, double* ms, uint64_t* launches, double* bytes) {
    return sfhe_sorter_graph_family_time(s, SFHE_KFAM_NTT, reps, ms, launches, bytes);
}

int sfhe_sorter_graph_nodes(const sfhe_sorter* s, uint64_t* nodes) {
    REQUIRE(s && nodes, "null argument");
    *nodes = s->impl->graphNodes();
    return SFHE_OK;
}

int sfhe_sorter_records_graph_nodes(const sfhe_sorter* s, uint64_t* nodes) {
    REQUIRE(s && nodes, "null argument");
    *nodes = s->impl->recordsGraphNodes();
    return SFHE_OK;
}

int sfhe_decompose(uint32_t N, const int32_t* keys, size_t nkeys, int32_t rotation, int32_t wrapN,
                   int algo, int32_t* values, int32_t* steps, size_t cap, size_t* count) {
    REQUIRE(validN(N) && keys && nkeys && wrapN > 0, "bad argument");
    std::vector<int> k(keys, keys + nkeys);
    return guard([&] {
        switch (N) {
#define CASE(K) \
    case K: decomposeN<K>(k, rotation, wrapN, algo, values, steps, cap, count); break;
            CASE(4) CASE(8) CASE(16) CASE(32) CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
        }
    });
}

int sfhe_debug_decrypt_coeffs(sfhe_ctx* c, const sfhe_ct* ct, double* out, size_t cap) {
    REQUIRE(c && ct && out, "null argument");
    REQUIRE(c->keys.secretKey, "no secret key");
    REQUIRE(!c->cc->IsSharded(), "debug decrypt needs an unsharded context");
    const size_t n = c->cc->GetRingDimension();
    REQUIRE(cap >= n, "output buffer too small");
    return guard([&] {
        auto* s = c->cc->state();
        c->cc->Settle(ct->ct);
        auto t = s->alloc(n);
        const sfp_limbs q{1, 1, 0, 0};
        sfp_mul_add(s->dev, t->ptr, ct->ct->c1, c->keys.secretKey->s->ptr, ct->ct->c0, q);
        sfp_ntt(s->dev, t->ptr, q, 1);
        std::vector<uint64_t> h(n);
        sfp_d2h(s->dev, h.data(), t->ptr, n * 8);
        const uint64_t q0 = s->primes[0];
        for (size_t i = 0; i < n; ++i) out[i] = h[i] > q0 / 2 ? -(double)(q0 - h[i]) : (double)h[i];
    });
}

int sfhe_kernel_timing(sfhe_ctx* c, uint32_t family, uint32_t period) {
    REQUIRE(c, "null context");
    REQUIRE(family < SFP_FAM_COUNT, "unknown kernel family");
    return guard([&] {
        OpLock g(c->cc->state());
        sfp_prof_set(c->cc->state()->dev, family, period);
    });
}

int sfhe_serialize_lanes(sfhe_ctx* c, int on) {
    REQUIRE(c, "null context");
    return guard([&] {
        OpLock g(c->cc->state());
        sfp_serialize(c->cc->state()->dev, on);
    });
}

int sfhe_stack_stats(sfhe_ctx* c, uint64_t* merged, uint64_t* single) {
    REQUIRE(c, "null context");
    return guard([&] {
        OpLock g(c->cc->state());
        sfp_stack_stats(c->cc->state()->dev, merged, single);
    });
}

int sfhe_comm_stats_reset(sfhe_ctx* c, int timed) {
    REQUIRE(c, "null context");
    return guard([&] {
        OpLock g(c->cc->state());
        sfp_comm_stats_reset(c->cc->state()->dev, timed);
    });
}

int sfhe_comm_stats(sfhe_ctx* c, uint64_t* calls, double* bytes, double* ms) {
    REQUIRE(c, "null context");
    return guard([&] {
        OpLock g(c->cc->state());
        sfp_comm_stats(c->cc->state()->dev, calls, bytes, ms);
    });
}

int sfhe_kernel_timing_read(sfhe_ctx* c, uint32_t family, uint64_t* launches, uint64_t* timed,
                            double* ms, double* bytes) {
    REQUIRE(c, "null context");
    REQUIRE(family < SFP_FAM_COUNT, "unknown kernel family");
    return guard([&] {
        OpLock g(c->cc->state());
        sfp_prof_read(c->cc->state()->dev, family, launches, timed, ms, bytes);
    });
}

int sfhe_context_primes(sfhe_ctx* c, uint64_t* out, size_t cap, size_t* count) {
    REQUIRE(c, "null context");
    const auto& p = c->cc->state()->primes;
    if (count) *count = p.size();
    for (size_t i = 0; i < p.size() && i < cap && out; ++i) out[i] = p[i];
    return SFHE_OK;
}

int sfhe_live_contexts(void) { return CryptoContextImpl<DCRTPoly>::LiveContexts(); }

int sfhe_pool_bytes(sfhe_ctx* c, uint64_t* bytes) {
    REQUIRE(c && bytes, "null argument");
    *bytes = c->cc->GetOpStats().pool_bytes;
    return SFHE_OK;
}

// ---- limb sharding ----
int sfhe_comm_uid(uint8_t uid[128]) {
    REQUIRE(uid, "null argument");
    if (sfp_comm_uid(uid) != 0) {
        g_err = std::string("no RCCL communicator in the ") + sfp_backend_name() + " backend";
        return SFHE_ENOTIMPL;
    }
    return SFHE_OK;
}

int sfhe_shard_rccl(sfhe_ctx* c, int rank, int world, const uint8_t uid[128]) {
    REQUIRE(c && uid, "null argument");
    REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
    REQUIRE(!c->keys.secretKey, "shard the context before sfhe_keygen");
    REQUIRE(!c->cc->IsSharded(), "context already sharded");
    return guard([&] {
        auto* s = c->cc->state();
        if (sfp_comm_init_rccl(s->dev, rank, world, uid) != 0) {
            const char* e = sfp_last_error(s->dev);
            throw OpenFHEException(std::string("device error: RCCL communicator: ") + (e ? e : "init failed"));
        }
        // a one-rank communicator runs the sharded path too: its all-gathers
        // and broadcasts go through RCCL (single-GPU validation)
        c->cc->EnableSharding(rank, world, true);
    });
}

int sfhe_shard_host(sfhe_ctx* c, int rank, int world, sfhe_allgather_fn ag, sfhe_bcast_fn bc, void* user) {
    REQUIRE(c && ag && bc, "null argument");
    REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
    REQUIRE(!c->keys.secretKey, "shard the context before sfhe_keygen");
    REQUIRE(!c->cc->IsSharded(), "context already sharded");
    return guard([&] {
        c->cc->EnableSharding(rank, world);
        sfp_comm_set_host(c->cc->state()->dev, rank, world, ag, bc, user);
    });
}

int sfhe_shard_tail(const sfhe_ctx* c, uint32_t* limbs) {
    REQUIRE(c && limbs, "null argument");
    *limbs = c->cc->ShardTailLimbs();
    return SFHE_OK;
}

int sfhe_key_rows(const sfhe_ctx* c, uint32_t* rows) {
    REQUIRE(c && rows, "null argument");
    *rows = c->cc->SwitchKeyRows();
    return SFHE_OK;
}

// ---- batch groups ----
int sfhe_groups_rccl(sfhe_ctx* c, int group, int groups, const uint8_t uid[128]) {
    REQUIRE(c && uid, "null argument");
    REQUIRE(groups >= 1 && group >= 0 && group < groups, "bad group / groups");
    REQUIRE(!c->keys.secretKey, "set the batch groups before sfhe_keygen");
    REQUIRE(c->cc->BatchGroups() == 1, "batch groups already set");
    return guard([&] {
        auto* s = c->cc->state();
        if (sfp_group_init_rccl(s->dev, group, groups, uid) != 0) {
            const char* e = sfp_last_error(s->dev);
            throw OpenFHEException(std::string("device error: RCCL group communicator: ") +
                                   (e ? e : "init failed"));
        }
        // a one-group communicator still gathers every part (through RCCL)
        c->cc->EnableBatchGroups(group, groups, true);
    });
}

int sfhe_groups_host(sfhe_ctx* c, int group, int groups, sfhe_allgather_fn ag, void* user) {
    REQUIRE(c && ag, "null argument");
    REQUIRE(groups >= 1 && group >= 0 && group < groups, "bad group / groups");
    REQUIRE(!c->keys.secretKey, "set the batch groups before sfhe_keygen");
    REQUIRE(c->cc->BatchGroups() == 1, "batch groups already set");
    return guard([&] {
        c->cc->EnableBatchGroups(group, groups, true);
        sfp_group_set_host(c->cc->state()->dev, group, groups, ag, user);
    });
}

int sfhe_groups(const sfhe_ctx* c, int* group, int* groups) {
    REQUIRE(c && group && groups, "null argument");
    *group = c->cc->BatchGroup();
    *groups = c->cc->BatchGroups();
    return SFHE_OK;
}

}  // extern "C"
