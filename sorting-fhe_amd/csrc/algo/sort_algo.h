// Encrypted rank sort ("Optimized Rank Sort") on the device engine.
//
// Public surface of the reference's src/sort_algo.h: SortAlgo :22,
// SortBase<N> :36-59, DirectSort<N> :61-774 (getSizeParameters :87-201,
// slot-vector generators :206-306, vecRotsOpt :326-366, constructRank
// :368-506, blindRotationOptN :561-584, rotationIndexCheckN :658-750,
// sort :752-774) and BitonicSort<N> :1393-1487 (link-only here).
//
// Slot-level semantics, with P = min(N, n/2/N)
// partitions, B = N/P batches and S = N*P slots:
//   rank_r = sum_d step(x_r - x_{(r+d) mod N}) - 1/2  = #{j : x_j < x_r}
//   out[rank_r] = x_r, via the doubled-sinc indicator D((r - rank_r - c)/2N)
//   and per-partition masked rotations by c = (b*P + p) mod N.
//
// Engine extension, not in the reference: sortStable / constructRankStable,
// the tie-aware stable rank  #{j : x_j < x_r} + #{j < r : x_j = x_r}  for
// inputs with duplicate values (equal, or at least the sign's resolution
// apart), one level deeper.  Measured on the oracle, every
// multiplicity up to all-equal at N = 256 passes the 0.01 output gate
// (worst: 1.1e-3).  The reference-signature methods behave as before.
// Records: placeMany places several columns by one rank with
// the indicator evaluated once per batch, sortRecords = the (stable) rank of
// a key column + placeMany of the keys and their payload columns.
// Record selection: selectRanksMany / selectRecords select the
// rows of chosen ranks, likewise with one indicator per batch for all columns.
// Several keys: constructRankLex ranks rows in (key_1, ...,
// key_m, input index) order in one pass; sortRecordsLex / selectRecordsLex
// place / select the keys and payload columns by it.
// Grouping: groupAggregate gives every row the size of its
// key's group, its number inside the group and the group's column sums.
// Window sums: windowSums gives every row, in input order, the
// running count and column sums over the rows before it in key order.
// Join: joinAggregate gives every row of a table A the number
// of rows of a table B that agree with it on up to SFHE_LEX_KEYS keys, and B's
// column sums over them.
// What these methods share is written once: runBatches (the batches over
// lanes and batch groups), sumOverPartitions (batch sum and folds),
// sfhe::SincIndicator (the placements' and selections' indicator), MemoTag and
// memoPlain with the entries' builders, lexRank (the stable rank is its
// one-key case) and runCached (the graph protocol of the plain, the stable
// and the record sort).
//
// Engine-specific scheduling (identical slot values, fewer key switches):
//   * baby-step rotations of one ciphertext share one hoisted ModUp;
//   * each giant step's sum of np plaintext-mask products is accumulated
//     before a single rescale (MultAddPlain), instead of np rescales.
#pragma once

#include <algorithm>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <map>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <iostream>
#include <string>
#include <tuple>
#include <vector>

#include "ciphertext-fwd.h"
#include "coefficients.h"
#include "comparison.h"
#include "encryption.h"
#include "size_params.h"
#include "lattice/hal/lat-backend.h"
#include "mehp24/mehp24_utils.h"
#include "openfhe.h"
#include "rotation.h"

using namespace lbcrypto;

enum class SortAlgo { DirectSort, BitonicSort };

inline void printElapsedTime(const std::string& what,
                             const std::chrono::high_resolution_clock::time_point& start) {
    auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                  std::chrono::high_resolution_clock::now() - start)
                  .count();
    std::cout << what << ": " << ms << " ms" << std::endl;
}

namespace sfhe {

inline int ilog2(long v) {
    int r = 0;
    while ((1L << (r + 1)) <= v) ++r;
    return r;
}

// Per-N metadata shared by constructRank and rotationIndexCheckN.
struct RankLayout {
    int N, P, B, S, npRank, npPlace;
    RankLayout(int N, int maxBatch) : N(N) {
        P = std::min(N, maxBatch / N);
        B = N / P;
        S = N * P;
        // baby-step counts: 2^floor(log2(N)/2), as the reference's tables
        // (sort_algo.h:383-416, :670-703)
        npRank = std::min(1 << (ilog2(N) / 2), P);
        npPlace = N <= 256 ? (1 << (ilog2(N) / 2)) : (N <= 1024 ? 8 : 4);
    }
};

// Sign configuration DirectSortTest uses for each N (DirectSortTest.cpp:113-121).
inline CompositeSignConfig defaultSignConfig(int N) {
    if (N <= 16) return CompositeSignConfig(3, 2, 2);
    if (N <= 128) return CompositeSignConfig(3, 3, 2);
    if (N <= 512) return CompositeSignConfig(3, 4, 2);
    return CompositeSignConfig(3, 5, 2);
}

// Levels consumed by DirectSort::sort with sign config `c`:
//   rank: 1 (mask) + 3 * (max(dg,1) + df) (n = 3) + 1 (x 1/2)
//   placement: 1 (x 1/2N) + PS depth of the doubled sinc + 1 (x input) + 1 (mask)
inline int compositeSignDepth(const CompositeSignConfig& c) {
    if (c.n == 4) return 5 * std::max(c.dg, 1) + 4 * c.df;
    return (c.n == 3 ? 3 : 0) * (std::max(c.dg, 1) + c.df);
}
inline int directSortDepth(int N, const CompositeSignConfig& c) {
    const int sign = compositeSignDepth(c);
    const int ps = (int)lbcrypto::ChebyshevPSDepth(
        (uint32_t)sfhe::doubledSincCoefficients(N).size() - 1);
    return 1 + sign + 1 + 1 + ps + 1 + 1;
}
// The stable (tie-aware) sort: the rank's x 1/2 becomes the tie term
// s (.) (W (.) s + 1/2), degree 2 in the sign with one plaintext factor --
// one level more; the placement is unchanged.
//   rank: 1 (mask) + sign + 2 (tie term)
inline int stableRankDepth(const CompositeSignConfig& c) { return 1 + compositeSignDepth(c) + 2; }
inline int stableSortDepth(int N, const CompositeSignConfig& c) { return directSortDepth(N, c) + 1; }
// The lexicographic sort by m keys: every key's tie term, then
// one Horner step (EvalLexStep, one level) per key after the first.
#define SFHE_LEX_KEYS 4
inline int lexRankDepth(const CompositeSignConfig& c, int m) { return stableRankDepth(c) + (m - 1); }
inline int lexSortDepth(int N, const CompositeSignConfig& c, int m) { return stableSortDepth(N, c) + (m - 1); }
// Grouping by a key: 1 (mask) + sign + 1 (q = s^2) + 1 (the
// gated product, or the index mask): the stable rank's levels and no placement.
inline int groupDepth(const CompositeSignConfig& c) { return stableRankDepth(c); }
// Window sums over an ordered frame: the stable rank's tie
// term as the gate, then 1 (the gated product); no placement.
inline int windowDepth(const CompositeSignConfig& c) { return stableRankDepth(c) + 1; }
// Join of two tables on m keys: the grouping's levels, and
// the balanced tree of EvalGateOr over the keys' gates (one level per layer).
inline int joinDepth(const CompositeSignConfig& c, int m) {
    int layers = 0;
    while ((1 << layers) < m) ++layers;
    return groupDepth(c) + layers;
}

// getSizeParameters' (depth, rotation keys) for N (reference :87-201);
// nullptr when the reference has no entry.
inline const SizeParams* sizeParams(int N) {
    for (const auto& e : sizeParamTable())
        if (e.N == N) return &e;
    return nullptr;
}

}  // namespace sfhe

// ---------------------------------------------------------------------------
namespace sfhe {
// Runs body(b) for b < count, batch b on lane b % lanes.  By default one host
// thread issues the batches in order (the GPU already overlaps the lanes:
// issuing is ~3x faster than the device work).  SFHE_HOST_THREADS=1 gives
// each lane its own host thread (the reference's OpenMP batch loop); the
// first exception is rethrown after all threads join.
inline bool hostThreads() {
    static const bool on = [] {
        const char* v = std::getenv("SFHE_HOST_THREADS");
        return v && *v && *v != '0';
    }();
    return on;
}

template <class F>
void parallelLanes(const CryptoContext<DCRTPoly>& cc, int lanes, int count, F&& body) {
    if (!hostThreads() || lanes <= 1) {
        for (int b = 0; b < count; ++b) {
            cc->SetLane(b % lanes);
            body(b);
        }
        cc->SetLane(0);
        return;
    }
    std::exception_ptr err;
    std::mutex em;
    auto run = [&](int t) {
        try {
            cc->SetLane(t);
            for (int b = t; b < count; b += lanes) body(b);
        } catch (...) {
            std::lock_guard<std::mutex> g(em);
            if (!err) err = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < lanes; ++t) th.emplace_back(run, t);
    run(0);
    for (auto& x : th) x.join();
    cc->SetLane(0);
    if (err) std::rethrow_exception(err);
}

// The batches of one sort phase over the context's batch groups (DESIGN.md
// §7): group g of G runs the batches b with b % G == g; gatherParts then
// all-gathers every part over the group communicator, so each rank holds all
// B parts and sums them exactly as an unsplit sort.  The parts are settled
// (canonical) on every path, split or not, so the sums are bit-identical.
// B not a multiple of G: every group runs every batch (no split).  A
// one-group communicator (BatchGather at G = 1) still routes every part
// through the collective: single-GPU validation.
struct BatchSplit {
    int G = 1, g = 0;
    bool gather = false;
    std::vector<int> mine;
    BatchSplit(const CryptoContext<DCRTPoly>& cc, int B) {
        if (cc->BatchGroups() > 1 && B % cc->BatchGroups() == 0) {
            G = cc->BatchGroups();
            g = cc->BatchGroup();
            gather = true;
        } else if (cc->BatchGroups() == 1) {
            gather = cc->BatchGather();
        }
        for (int b = g; b < B; b += G) mine.push_back(b);
    }
    void gatherParts(const CryptoContext<DCRTPoly>& cc, std::vector<Ciphertext<DCRTPoly>>& parts) const {
        if (!gather) {
            for (auto& p : parts) cc->Settle(p);
            return;
        }
        for (size_t k = 0; k < parts.size() / G; ++k) {
            auto all = cc->GatherGroups(parts[k * G + g]);
            for (int h = 0; h < G; ++h) parts[k * G + h] = all[h];
        }
    }
};

// The batches of a sort phase run the same op sequence on their lanes.
// SFHE_STACK_BATCHES=1 issues them as stacked launches (one launch per op for
// both batches, ForkLanes(k, true)); by default they run on two streams that
// overlap on the device, which measured faster (47.3 vs 57.0 ms).
inline bool stackBatches() {  // (read per sort phase: tests switch it)
    const char* v = std::getenv("SFHE_STACK_BATCHES");
    return v && *v == '1';
}

// Placement evaluates the doubled sinc in the rebased variable (on unless
// SFHE_SINC_REBASE=0; see SincIndicator).
inline bool sincRebase() {
    const char* v = std::getenv("SFHE_SINC_REBASE");
    return !v || *v != '0';
}

// constructRank moves the self comparison off the sign's steep point (on
// unless SFHE_SELF_OFFSET=0, which computes step(0) = 1/2 as the reference).
constexpr double kSelfOffset = 0.5;
inline bool selfOffset() {
    static const bool on = [] {
        const char* v = std::getenv("SFHE_SELF_OFFSET");
        return !v || *v != '0';
    }();
    return on;
}

// SFHE_PHASES=1: device-synchronised wall time of each sort phase on stderr
// (diagnostics only; adds synchronisation, so never on in benchmarks).
class PhaseTimer {
  public:
    explicit PhaseTimer(CryptoContext<DCRTPoly> cc) : m_cc(std::move(cc)) {
        static const bool on = std::getenv("SFHE_PHASES") != nullptr;
        m_on = on;
        if (m_on) {
            m_cc->Synchronize();
            m_t = std::chrono::steady_clock::now();
            m_s = m_cc->GetOpStats();
        }
    }
    void mark(const char* what) {
        if (!m_on) return;
        std::lock_guard<std::mutex> g(m_mu);  // lanes on host threads mark too
        m_cc->Synchronize();
        auto now = std::chrono::steady_clock::now();
        const auto st = m_cc->GetOpStats();
        // op counts since the last mark: key switches, rescales, ct x ct
        // tensors, automorphisms and NTT limb-transforms
        std::fprintf(stderr, "PHASE %-36s %8.3f ms  ks %4llu  rs %4llu  tensor %4llu  aut %4llu  ntt %6llu\n",
                     what, std::chrono::duration<double, std::milli>(now - m_t).count(),
                     (unsigned long long)(st.keyswitch - m_s.keyswitch), (unsigned long long)(st.rescale - m_s.rescale),
                     (unsigned long long)(st.tensor - m_s.tensor), (unsigned long long)(st.automorph - m_s.automorph),
                     (unsigned long long)(st.ntt_limbs - m_s.ntt_limbs));
        m_t = now;
        m_s = st;
    }

  private:
    CryptoContext<DCRTPoly> m_cc;
    bool m_on = false;
    std::mutex m_mu;
    std::chrono::steady_clock::time_point m_t;
    CryptoContextImpl<DCRTPoly>::OpStats m_s;
};

// The indicator of both placements and both selections, one value per call:
// D(d / 2N) of an integer offset d in (-2N, N) is 1 at d = 0 and 0 at the
// other integers.  The doubled sinc p is evaluated on y = (4z + 1)/3, its
// argument's range z = d/2N in (-1, 1/2) mapped onto [-1, 1]: the same
// polynomial (re-expanded, sfhe::rebasedChebyshev), the same levels, but the
// hits z = 0 land at y = 1/3 instead of an extremum of every giant step
// T_{2^i}, which cuts the CKKS noise of the placement ~2^8-fold (DESIGN.md
// §2).  SFHE_SINC_REBASE=0 evaluates p(z) as the reference.
struct SincIndicator {
    int N;
    bool rebase;
    const std::vector<double>& coeffs;
    double zmul, zadd;
    uint32_t psDepth;  // the PS depth of the reference's series (level tables)
    explicit SincIndicator(int N)
        : N(N), rebase(sincRebase()),
          coeffs(rebase ? rebasedChebyshev(doubledSincCoefficients(N), -1.0, 0.5) : doubledSincCoefficients(N)),
          zmul(rebase ? 4.0 / 3.0 : 1.0), zadd(rebase ? 1.0 / 3.0 : 0.0),
          psDepth(lbcrypto::ChebyshevPSDepth((uint32_t)doubledSincCoefficients(N).size() - 1)) {}
    // hit = D(diff / 2N), diff the ciphertext of the offsets d
    Ciphertext<DCRTPoly> hit(const CryptoContext<DCRTPoly>& cc, const Ciphertext<DCRTPoly>& diff,
                             PhaseTimer& ph) const {
        auto z = cc->EvalMult(diff, zmul / N / 2);
        if (rebase) z = cc->EvalAdd(z, zadd);
        ph.mark("  indicator: z");
        auto h = cc->EvalChebyshevSeriesPS(z, coeffs, -1, 1);
        // the rebased series may be shorter (tiny tail terms dropped) and so
        // shallower: consume exactly the reference's PS depth (level tables)
        const uint32_t psLevel = z->GetLevel() + psDepth;
        if (h->GetLevel() < psLevel) h = cc->AdjustLevel(h, psLevel);
        ph.mark("  indicator: sinc PS");
        return h;
    }
};
}  // namespace sfhe

template <int N>
class SortBase {
  protected:
    std::shared_ptr<Encryption> m_enc;
    const Ciphertext<DCRTPoly> m_zeroCache;

    // fresh encryption of N zeros: the accumulator seed of every sum
    virtual Ciphertext<DCRTPoly> createZeroCache() {
        return m_enc->encryptInput(std::vector<double>(N, 0.0));
    }

  public:
    SortBase(std::shared_ptr<Encryption> enc) : m_enc(enc), m_zeroCache(createZeroCache()) {}
    virtual ~SortBase() = default;

    virtual Ciphertext<DCRTPoly> sort(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                      SignConfig& Cfg) = 0;

    virtual const Ciphertext<DCRTPoly>& getZero() const { return m_zeroCache; }
    constexpr size_t getArraySize() const { return N; }
};

template <int N>
class DirectSort : public SortBase<N> {
  private:
    CryptoContext<DCRTPoly> m_cc;
    PublicKey<DCRTPoly> m_PublicKey;
    Comparison comp;
    RotationComposer<N> rot;
    int max_batch;  // n/2

  public:
    std::shared_ptr<Encryption> m_enc;

    DirectSort(CryptoContext<DCRTPoly> cc, PublicKey<DCRTPoly> publicKey,
               std::vector<int> rotIndices, std::shared_ptr<Encryption> enc)
        : SortBase<N>(enc), m_cc(cc), m_PublicKey(publicKey), comp(enc),
          rot(m_cc, enc, rotIndices), max_batch((int)cc->GetRingDimension() / 2), m_enc(enc) {}

    const std::set<int>& getRotationCalls() const { return rot.getRotationCalls(); }

    // Batch size, scale, depth and rotation keys for this N (reference
    // :87-201; the tables are the reference's, sfhe::directSortDepth
    // re-derives the depths and tests/test_host.py checks they agree).
    static void getSizeParameters(CCParams<CryptoContextCKKSRNS>& parameters,
                                  std::vector<int>& rotations) {
        parameters.SetBatchSize(N);
        const sfhe::SizeParams* p = sfhe::sizeParams(N);
        if (!p) {
            std::cerr << "Unsupported N" << std::endl;
            std::exit(1);
        }
        parameters.SetScalingModSize(40);
        parameters.SetMultiplicativeDepth((uint32_t)p->multDepth);
        rotations = p->rotations;
    }

    // ---- slot-vector generators (reference :206-306) ----
    // 1 on partition k = slots [kN, (k+1)N)
    std::vector<double> generateMaskVector(int num_slots, int k) {
        std::vector<double> v(num_slots, 0.0);
        std::fill(v.begin() + (size_t)k * N, v.begin() + (size_t)(k + 1) * N, 1.0);
        return v;
    }
    std::vector<double> generateMaskVectorN(int num_slots, int k) {
        return generateMaskVector(num_slots, k);
    }
    std::vector<double> generateMaskVector2N(int num_slots, int k) {
        std::vector<double> v(num_slots, 0.0);
        std::fill(v.begin() + (size_t)2 * k * N, v.begin() + (size_t)2 * (k + 1) * N, 1.0);
        return v;
    }
    // [0, 1, ..., N-1]
    std::vector<double> generateIndexVector() {
        std::vector<double> v(N);
        for (int i = 0; i < N; ++i) v[i] = i;
        return v;
    }
    // partition p holds (k + p) mod N
    std::vector<double> generateCheckingVectorN(int num_slots, int k) {
        std::vector<double> v(num_slots);
        for (int s = 0; s < num_slots; ++s) v[s] = (k + s / N) % N;
        return v;
    }
    // blocks of 2N: N copies of c then N copies of c - N, c = (k + block) mod N
    std::vector<double> generateCheckingVector2N(int num_slots, int k) {
        std::vector<double> v(num_slots);
        for (int s = 0; s < num_slots; ++s) {
            int c = (k + s / (2 * N)) % N;
            v[s] = (s % (2 * N)) < N ? c : c - N;
        }
        return v;
    }
    // left rotation for r > 0, right rotation for r < 0
    std::vector<double> vectorRotate(const std::vector<double>& v, int r) {
        if (v.empty()) return {};
        const long n = (long)v.size();
        long s = ((r % n) + n) % n;
        std::vector<double> out(v.size());  // out[i] = v[(i + s) mod n]
        std::rotate_copy(v.begin(), v.begin() + s, v.end(), out.begin());
        return out;
    }

    // shifted[pN + r] = x[(r + is*P + p) mod N]: baby steps pre_i = Rot(x, i),
    // giant steps j: Rot(sum_i pre_i * RotR(mask_{np j + i}, is*P + j np), is*P + j np)
    // The 0/1 masks depend only on (N, layout, batch, giant step, level), so
    // their Plaintexts (and with them the device encodings) are kept across
    // sorts: repeated sorts skip mask generation, rotation and re-encoding.
    // A memo key is {tag, a, b, level, slots}; the tags' values are part of
    // the keys (a, b in brackets).
    enum MemoTag : int {
        kRankMasks = 0,          // vecRotsOpt's giant-step masks [is, j]
        kBlindMasks = 1,         // blindRotationMasks [0, i]
        kIndexVector = 2,        // indexPlain
        kCheckingVector = 3,     // checkingPlain [b]
        kColumnMask = 4,         // sumColumnsToTarget [M, column]
        kRowMask = 5,            // transposeColumnTarget [M, row]
        kHybrid1Sub = 6,         // matrixPlacement's subMask, hybrid I [b]
        kSelfOffset = 7,         // selfOffsetPlain
        kHybridSub = 8,          // matrixPlacement's subMask, hybrid and hybrid II [b]
        kBlindMasks2N = 9,       // blindRotationOpt2N [0, i]
        kCheckingVector2N = 10,  // rotationIndexCheck2N [b]
        kTieWeights = 11,        // tieWeightsPlain [b]
        kRankBase = 12,          // rankBasePlain [self offset on]
        kTargets = 13,           // targetPlain [b, target list]
        kMoveMasks = 14,         // moveMasks [target list, 1024 b + g]
        kBeforeMask = 15,        // groupAggregate's M_b [b]
        kGroupIndex = 16,        // groupAggregate's index vector
        kWindowWeights = 17,     // windowSums' W_b = -w_b [frame, b]
        kWindowGate = 18,        // windowSums' p_b = 1/2 + w_b [frame, b]
        kWindowCount = 19        // windowSums' K [frame]
    };
    std::map<std::array<int, 5>, std::vector<Plaintext>> m_masks;
    std::mutex m_masksMu;  // the batches' host threads share the memo
    // Returns the memoised plaintexts for `key`, building them once with
    // build(vec).  Filled under the lock; std::map references stay valid.
    template <class F>
    const std::vector<Plaintext>& maskMemo(const std::array<int, 5>& key, F&& build) {
        std::lock_guard<std::mutex> g(m_masksMu);
        auto& v = m_masks[key];
        if (v.empty()) build(v);
        return v;
    }
    // The memo entries of `keys`, `count` masks each, mask i of entry k made
    // by make(k, i); the missing ones built over the host's cores (the cold
    // sort's mask generation: 128 vectors of 32768 slots per giant-step
    // phase at the metric config).  Entries are filled in place, so the map
    // is not modified while the threads run.
    template <class F>
    std::vector<const std::vector<Plaintext>*> maskMemoMany(const std::vector<std::array<int, 5>>& keys, int count,
                                                            F&& make) {
        std::lock_guard<std::mutex> g(m_masksMu);
        std::vector<std::vector<Plaintext>*> vs;
        std::vector<std::pair<size_t, int>> todo;
        for (size_t k = 0; k < keys.size(); ++k) {
            auto& v = m_masks[keys[k]];
            if (v.empty()) {
                v.resize(count);
                for (int i = 0; i < count; ++i) todo.emplace_back(k, i);
            }
            vs.push_back(&v);
        }
        lbcrypto::ParallelFor(
            todo.size(), [&](size_t t) { (*vs[todo[t].first])[todo[t].second] = make(todo[t].first, todo[t].second); },
            2);
        return {vs.begin(), vs.end()};
    }
    // The memo entry {tag, a, b, level, slots} that holds one packed plaintext,
    // encoded from slotVector() the first time.
    template <class F>
    const Plaintext& memoPlain(MemoTag tag, int a, int b, uint32_t level, int slots, F&& slotVector) {
        return maskMemo({tag, a, b, (int)level, slots}, [&](auto& v) {
            v.push_back(m_cc->MakeCKKSPackedPlaintext(slotVector(), 1, level, nullptr, slots));
        })[0];
    }
    // [0, 1, ..., N-1] over N slots (the grouping keeps an entry of its own)
    const Plaintext& indexPlain(uint32_t level, MemoTag tag = kIndexVector) {
        return memoPlain(tag, 0, 0, level, N, [&] { return generateIndexVector(); });
    }
    // kSelfOffset on the self comparison's slots: partition 0 of batch 0
    const Plaintext& selfOffsetPlain(uint32_t level, int num_slots) {
        return memoPlain(kSelfOffset, 0, 0, level, num_slots, [&] {
            std::vector<double> o(num_slots, 0.0);
            std::fill(o.begin(), o.begin() + N, sfhe::kSelfOffset);
            return o;
        });
    }
    const Plaintext& tieWeightsPlain(int b, uint32_t level, const sfhe::RankLayout& L) {
        return memoPlain(kTieWeights, b, 0, level, L.S, [&] { return generateTieWeights(L.S, L.P, b); });
    }
    // The stable rank's constants: the terms' 1/2 + w sum to r over d != 0 and
    // the self slots give 1/2, less the self comparison (step(selfOffset) = 1,
    // the reference's step(0) = 1/2).
    const Plaintext& rankBasePlain(uint32_t level, bool offsetSelf) {
        return memoPlain(kRankBase, offsetSelf ? 1 : 0, 0, level, N, [&] {
            const double self = 0.5 - (offsetSelf ? 1.0 : 0.5);
            std::vector<double> c(N);
            for (int r = 0; r < N; ++r) c[r] = r + self;
            return c;
        });
    }
    const Plaintext& checkingPlain(int b, uint32_t level, const sfhe::RankLayout& L) {
        return memoPlain(kCheckingVector, b, 0, level, L.S, [&] { return generateCheckingVectorN(L.S, b * L.P); });
    }

    // [0, 1, ..., n-1]: the baby steps' rotation amounts
    static std::vector<int> babySteps(int n) {
        std::vector<int> amounts(n);
        for (int i = 0; i < n; ++i) amounts[i] = i;
        return amounts;
    }
    // the rank's baby-step rotations of one column, at S slots
    std::vector<Ciphertext<DCRTPoly>> rankBabyRotations(const Ciphertext<DCRTPoly>& x, const sfhe::RankLayout& L) {
        auto pre = rot.rotateMany(x, babySteps(L.npRank));
        for (auto& p : pre) p->SetSlots(L.S);
        return pre;
    }

    // Runs body(b) for the batches b < count of one phase.  The batches are
    // independent: each runs on its own lane (stream), and over batch groups
    // on its own GPU group (this group's share only).  The caller gathers its
    // parts with the split that is returned.
    template <class F>
    sfhe::BatchSplit runBatches(int count, F&& body) {
        sfhe::BatchSplit split(m_cc, count);
        const int lanes = std::min((int)split.mine.size(), m_cc->LaneCount());
        if (lanes > 1) m_cc->ForkLanes(lanes, sfhe::stackBatches());  // (one batch: no region, the PS may open its own)
        sfhe::parallelLanes(m_cc, lanes, (int)split.mine.size(), [&](int i) { body(split.mine[i]); });
        m_cc->JoinLanes();
        return split;
    }
    // The end of every batched phase: the parts added to `acc` in batch order,
    // then the sum over the partitions (period N inside S slots) by doubling
    // rotations, and N slots again.
    Ciphertext<DCRTPoly> sumOverPartitions(Ciphertext<DCRTPoly> acc, const std::vector<Ciphertext<DCRTPoly>>& parts,
                                           int S) {
        for (const auto& p : parts) m_cc->EvalAddInPlace(acc, p);
        for (int s = S / 2; s >= N; s /= 2) m_cc->EvalAddInPlace(acc, rot.rotate(acc, s));
        acc->SetSlots(N);
        return acc;
    }

    // The giant steps' rotations is*P + j*np are applied as one rotation by
    // is*P of the sum over j of rotations by j*np (rotations are linear), and
    // that sum shares one ModDown (rotateSum, output aggregation): per batch
    // P/np key switches with one ModDown instead of up to 2 P/np of each.
    Ciphertext<DCRTPoly> vecRotsOpt(const std::vector<Ciphertext<DCRTPoly>>& pre,
                                    int num_partition, int num_slots, int np, int is) {
        std::vector<std::array<int, 5>> keys;
        std::vector<int> steps;
        for (int j = 0; j < num_partition / np; ++j) {
            keys.push_back({kRankMasks, is, j, (int)pre[0]->GetLevel(), num_slots});
            steps.push_back(j * np);
        }
        const auto masks = maskMemoMany(keys, np, [&](size_t j, int i) {
            const int shift = is * num_partition + (int)j * np;
            return m_cc->MakeCKKSPackedPlaintext(vectorRotate(generateMaskVector(num_slots, np * (int)j + i), -shift),
                                                 1, pre[i]->GetLevel(), nullptr, num_slots);
        });
        std::vector<Ciphertext<DCRTPoly>> giants;
        for (const auto* m : masks) {  // T_j = sum_i pre_i * mask_{np j + i}
            giants.push_back(m_cc->EvalMultAddPlain(pre, *m));
            giants.back()->SetSlots(num_slots);
        }
        return rot.rotate(rot.rotateSum(giants, steps), is * num_partition);
    }

    // The self comparison x_r vs x_r sits in partition 0 of batch 0 (shift 0).
    // Its difference is pure CKKS noise at the composite sign's steepest
    // point (slope ~ 4.5^dg), which made it the largest term of the rank
    // error (~1e-4 at N=256).  The engine moves those N slots' difference to
    // +selfOffset (an exact plaintext addition, selfOffsetPlain), where the
    // sign is saturated: the term contributes 1 instead of 1/2 and the final
    // correction is -1 instead of the reference's -1/2 (:503-504).  Same rank
    // up to the sign's approximation error; DESIGN.md §2.
    Ciphertext<DCRTPoly> constructRank(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                       SignConfig& Cfg) {
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        const auto pre = rankBabyRotations(input_array, L);
        ph.mark("rank: baby rotations");
        auto rank = this->getZero()->Clone();
        rank->SetSlots(L.S);
        const bool offsetSelf = sfhe::selfOffset();
        std::vector<Ciphertext<DCRTPoly>> parts(L.B);
        const auto split = runBatches(L.B, [&](int b) {
            auto shifted = vecRotsOpt(pre, L.P, L.S, L.npRank, b);
            ph.mark("  rank batch: vecRotsOpt");
            auto dup = input_array->Clone();
            dup->SetSlots(L.S);
            if (b == 0 && offsetSelf) dup = m_cc->EvalAdd(dup, selfOffsetPlain(dup->GetLevel(), L.S));
            parts[b] = comp.compare(m_cc, dup, shifted, SignFunc, Cfg);
            ph.mark("  rank batch: compare");
        });
        split.gatherParts(m_cc, parts);
        rank = sumOverPartitions(rank, parts, L.S);
        ph.mark("rank: batch sum + folds");
        // remove the self comparison: step(selfOffset) = 1 (reference: step(0) = 1/2)
        return m_cc->EvalSub(rank, offsetSelf ? 1.0 : 0.5);
    }

    // The stable ascending rank #{j : x_j < x_r} + #{j < r : x_j = x_r}: correct
    // with duplicate values, equal keys keeping their input order (DESIGN.md
    // §4e).  Slot pN + r of batch b compares x_r with x_j, j = (r + d) mod N,
    // d = bP + p; with s the sign of x_r - x_j, e = 1 - s^2 marks a tie and
    //   t = 1/2 + s/2 + w e = (1/2 + w) + s (.) (1/2 - w (.) s),
    //   w = +1/2 where r + d >= N (j < r), -1/2 where r + d < N, 0 where d = 0
    // counts a tie exactly when j < r.  Per batch the variable part
    // s (.) (W (.) s + 1/2), W = -w, is one EvalTieTerm; the constants
    // 1/2 + w sum to r over d != 0 and are added once after the fold, with the
    // self comparison's correction.  One level more than constructRank.  It is
    // the lexicographic rank by one ascending key (lexRank).
    // Precondition: two inputs are equal or at least the sign configuration's
    // resolution apart (1/N for the default configurations).
    Ciphertext<DCRTPoly> constructRankStable(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                             SignConfig& Cfg) {
        const int need = (int)input_array->GetLevel() + sfhe::stableRankDepth(Cfg.compos);
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("stable rank: needs multiplicative depth " + std::to_string(need) +
                                   " (one level more than the plain rank for the tie term); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
        return lexRank({input_array}, {false}, SignFunc, Cfg);
    }

    // W = -w of batch b (constructRankStable)
    std::vector<double> generateTieWeights(int num_slots, int num_partition, int b) {
        std::vector<double> v(num_slots, 0.0);
        for (int p = 0; p < num_slots / N; ++p) {
            const int d = b * num_partition + p;
            if (d == 0) continue;
            for (int r = 0; r < N; ++r) v[(size_t)p * N + r] = r + d >= N ? -0.5 : 0.5;
        }
        return v;
    }

    // The lexicographic stable rank by m = keys.size() keys (1 <= m <=
    // SFHE_LEX_KEYS), key i descending where descending[i]: the number of j
    // before r in (key_1, ..., key_m, input index) order.  In
    // constructRankStable's slot layout, with s_i the sign of key i's
    // difference, v_i = s_i (.) (1/2 - w (.) s_i) its tie term and e_i = 1 -
    // s_i^2 its "equal on this key",
    //   t = (1/2 + w) + v_1 + e_1 (.) (v_2 + e_2 (.) (v_3 + ...)):
    // where key 1 differs t = 1/2 + s_1/2, where it ties t is key 2's stable
    // term, and so on down to the index.  Per batch: the m signs, the m tie
    // terms (EvalTieTerm), q_i = s_i^2 for i < m in one EvalMultMany, then the
    // Horner steps from the last key inwards (EvalLexStep, one level each):
    // m - 1 levels below constructRankStable, whose rank is the case m = 1 (no
    // product, no Horner step).  A descending key swaps the operands of its
    // difference.  The self offset goes on the first key's difference only
    // (+kSelfOffset whatever its direction), so s_1 = 1 and e_1 ~ 0 in the self
    // slots and the constants (rankBasePlain) do not depend on m.
    // Precondition per key: two values are equal or at least the sign
    // configuration's resolution apart.
    Ciphertext<DCRTPoly> constructRankLex(const std::vector<Ciphertext<DCRTPoly>>& keys,
                                          const std::vector<bool>& descending, SignFunc SignFunc, SignConfig& Cfg) {
        const int m = (int)keys.size();
        if (m < 1 || m > SFHE_LEX_KEYS)
            throw OpenFHEException("lexicographic rank: " + std::to_string(m) + " keys (1 .. " +
                                   std::to_string(SFHE_LEX_KEYS) + " are supported)");
        if ((int)descending.size() != m)
            throw OpenFHEException("lexicographic rank: one descending flag per key is needed");
        for (const auto& k : keys)
            if (k->GetLevel() != keys[0]->GetLevel() || k->GetSlots() != keys[0]->GetSlots())
                throw OpenFHEException("lexicographic rank: the keys must be at one level and slot count");
        const int need = (int)keys[0]->GetLevel() + sfhe::lexRankDepth(Cfg.compos, m);
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("lexicographic rank: needs multiplicative depth " + std::to_string(need) +
                                   " (the stable rank's, and one level per key after the first); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
        return lexRank(keys, descending, SignFunc, Cfg);
    }

    // constructRankLex's computation, after its checks
    Ciphertext<DCRTPoly> lexRank(const std::vector<Ciphertext<DCRTPoly>>& keys, const std::vector<bool>& descending,
                                 SignFunc SignFunc, SignConfig& Cfg) {
        const int m = (int)keys.size();
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> pre(m);
        for (int k = 0; k < m; ++k) pre[k] = rankBabyRotations(keys[k], L);
        ph.mark("lex rank: baby rotations");
        auto rank = this->getZero()->Clone();
        rank->SetSlots(L.S);
        const bool offsetSelf = sfhe::selfOffset();
        std::vector<Ciphertext<DCRTPoly>> parts(L.B);
        const auto split = runBatches(L.B, [&](int b) {
            std::vector<Ciphertext<DCRTPoly>> s(m), v(m);
            for (int k = 0; k < m; ++k) {
                // minuend - subtrahend: x_r - x_j ascending, x_j - x_r descending
                auto shifted = vecRotsOpt(pre[k], L.P, L.S, L.npRank, b);
                auto dup = keys[k]->Clone();
                dup->SetSlots(L.S);
                auto minuend = descending[k] ? shifted : dup;
                const auto& subtrahend = descending[k] ? dup : shifted;
                if (k == 0 && b == 0 && offsetSelf)
                    minuend = m_cc->EvalAdd(minuend, selfOffsetPlain(dup->GetLevel(), L.S));
                s[k] = sign(m_cc->EvalSub(minuend, subtrahend), m_cc, SignFunc, Cfg);
            }
            ph.mark("  lex rank batch: vecRotsOpt + signs");
            const Plaintext& W = tieWeightsPlain(b, s[0]->GetLevel(), L);
            for (int k = 0; k < m; ++k) v[k] = m_cc->EvalTieTerm(s[k], W, 0.5);
            auto u = v[m - 1];
            if (m > 1) {
                const std::vector<Ciphertext<DCRTPoly>> head(s.begin(), s.end() - 1);
                const auto q = m_cc->EvalMultMany(head, head);
                for (int k = m - 2; k >= 0; --k) u = m_cc->EvalLexStep(v[k], q[k], u);
            }
            parts[b] = u;
            ph.mark("  lex rank batch: tie terms + Horner steps");
        });
        split.gatherParts(m_cc, parts);
        rank = sumOverPartitions(rank, parts, L.S);
        ph.mark("lex rank: batch sum + folds");
        return m_cc->EvalAdd(rank, rankBasePlain(rank->GetLevel(), offsetSelf));
    }

    // ---- grouping by an encrypted key (COUNT(*), SUM(col), ROW_NUMBER() OVER
    // (PARTITION BY key)) ----
    struct GroupResult {
        Ciphertext<DCRTPoly> count;              // count_r = #{j : key_j = key_r}
        Ciphertext<DCRTPoly> index;              // index_r = #{j < r : key_j = key_r}; null unless asked for
        std::vector<Ciphertext<DCRTPoly>> sums;  // sums[c]_r = sum of cols[c]_j over {j : key_j = key_r}
    };
    // M_b of the grouping's index: 1 where r + d >= N (j < r), d = bP + p; 0 for all of d = 0
    std::vector<double> generateBeforeMask(int num_slots, int num_partition, int b) {
        std::vector<double> v(num_slots, 0.0);
        for (int p = 0; p < num_slots / N; ++p) {
            const int d = b * num_partition + p;
            for (int r = std::max(N - d, 0); r < N && d > 0; ++r) v[(size_t)p * N + r] = 1.0;
        }
        return v;
    }
    // In constructRank's slot layout (slot pN + r of batch b compares row r
    // with row j = (r + d) mod N, d = bP + p), with s_b the composite sign of
    // key_r - key_j, q_b = s_b^2 ("the keys differ") and u_bc column c's value at
    // row j in the same layout:
    //   count_r  = N - fold(sum_b q_b)_r                    at q's level
    //   sum_cr   = fold(sum_b (1 - q_b) (.) u_bc)_r          one level below q
    //   index_r  = r - fold(sum_b M_b (.) q_b)_r             one level below q
    // fold: the rank's sum over the P partitions, then SetSlots(N).  No self
    // offset here, whatever SFHE_SELF_OFFSET says: the self slot is a tie like
    // any other, its gate 1 - q is 1 up to the square of the sign's noise, so
    // the row's own value enters its sum with no special case.  Per batch on
    // its lane: vecRotsOpt of the key and of every column (the columns share the
    // key's masks), the sign, q_b, and M_b (.) q_b when the index is wanted;
    // after the join ONE EvalGateSumMany for all batches and columns, the sums
    // of q_b, and the folds.  The folds are the rank's doubling folds for every
    // output: log2 P rotations each by amounts the rank already has keys for,
    // where foldPartitions' radix-4 amounts would need keys of their own and
    // sum inside a partition, not across them.  Depth groupDepth: the stable
    // rank's.  Eager (no graph).  Precondition: two keys are equal or at least
    // the sign configuration's resolution apart.
    GroupResult groupAggregate(const Ciphertext<DCRTPoly>& keys, const std::vector<Ciphertext<DCRTPoly>>& cols,
                               SignFunc SignFunc, SignConfig& Cfg, bool wantIndex, size_t maxCols) {
        const size_t C = cols.size();
        if (C > maxCols)
            throw std::invalid_argument("group: " + std::to_string(C) + " payload columns (at most " +
                                        std::to_string(maxCols) + ")");
        for (const auto& c : cols)
            if (c->GetLevel() != keys->GetLevel() || c->GetSlots() != keys->GetSlots())
                throw std::invalid_argument("group: the key and the columns must be at one level and slot count");
        const int need = (int)keys->GetLevel() + sfhe::groupDepth(Cfg.compos);
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("group: needs multiplicative depth " + std::to_string(need) +
                                   " (the stable rank's: the sign, its square and the gated product); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        const auto pre = rankBabyRotations(keys, L);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> preCols(C);
        for (size_t c = 0; c < C; ++c) preCols[c] = rankBabyRotations(cols[c], L);
        ph.mark("group: baby rotations");

        std::vector<Ciphertext<DCRTPoly>> q(L.B), mq(wantIndex ? L.B : 0);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> u(C, std::vector<Ciphertext<DCRTPoly>>(L.B));
        const auto split = runBatches(L.B, [&](int b) {
            auto shifted = vecRotsOpt(pre, L.P, L.S, L.npRank, b);
            for (size_t c = 0; c < C; ++c) u[c][b] = vecRotsOpt(preCols[c], L.P, L.S, L.npRank, b);
            ph.mark("  group batch: vecRotsOpt");
            auto dup = keys->Clone();
            dup->SetSlots(L.S);
            auto s = sign(m_cc->EvalSub(dup, shifted), m_cc, SignFunc, Cfg);
            q[b] = m_cc->EvalMult(s, s);
            if (wantIndex) {
                const Plaintext& M = memoPlain(kBeforeMask, b, 0, q[b]->GetLevel(), L.S,
                                               [&] { return generateBeforeMask(L.S, L.P, b); });
                mq[b] = m_cc->EvalMult(q[b], M);
            }
            ph.mark("  group batch: sign + gate");
        });
        split.gatherParts(m_cc, q);
        if (wantIndex) split.gatherParts(m_cc, mq);
        for (auto& col : u) split.gatherParts(m_cc, col);
        ph.mark("group: batches");

        auto fold = [&](Ciphertext<DCRTPoly> x) {
            x->SetSlots(L.S);
            return sumOverPartitions(x, {}, L.S);
        };
        auto sumOf = [&](const std::vector<Ciphertext<DCRTPoly>>& parts) {
            auto acc = parts[0]->Clone();
            for (int b = 1; b < L.B; ++b) m_cc->EvalAddInPlace(acc, parts[b]);
            return acc;
        };
        GroupResult out;
        if (C) {
            out.sums = m_cc->EvalGateSumMany(q, u);
            for (auto& x : out.sums) x = fold(x);
        }
        ph.mark("group: gated sums + folds");
        out.count = m_cc->EvalSub((double)N, fold(sumOf(q)));
        if (wantIndex) {
            auto before = fold(sumOf(mq));
            out.index = m_cc->EvalSub(indexPlain(before->GetLevel(), kGroupIndex), before);
        }
        ph.mark("group: count + index");
        return out;
    }

    // ---- aggregates over an ordered frame (SUM(col) OVER (ORDER BY key),
    // ROW_NUMBER(), RANK(), CUME_DIST()) ----
    enum WindowFrame : int {
        kFrameRows = 0,   // (key_j, j) <= (key_r, r): ROWS UNBOUNDED PRECEDING .. CURRENT ROW in stable order
        kFrameRange = 1,  // key_j <= key_r: SQL's default frame, peers included
        kFrameBelow = 2   // key_j < key_r
    };
    struct WindowResult {
        Ciphertext<DCRTPoly> count;              // count_r = #{j in row r's frame}; null unless asked for
        std::vector<Ciphertext<DCRTPoly>> sums;  // sums[c]_r = sum of cols[c]_j over row r's frame
    };
    // w of the frame in slot pN + r of batch b (d = bP + p, j = (r + d) mod N):
    // a tie counts where w = +1/2 and does not where w = -1/2
    static double windowWeight(int frame, int r, int d) {
        if (frame == kFrameRange) return 0.5;
        if (frame == kFrameBelow) return -0.5;
        return d == 0 || r + d >= N ? 0.5 : -0.5;  // rows: the self slot and j < r
    }
    // sign * w (sign = -1: W_b) or 1/2 + w (sign = 0: p_b) over batch b's slots
    std::vector<double> generateWindowWeights(int num_slots, int num_partition, int b, int frame, int sign) {
        std::vector<double> v(num_slots);
        for (int p = 0; p < num_slots / N; ++p)
            for (int r = 0; r < N; ++r) {
                const double w = windowWeight(frame, r, b * num_partition + p);
                v[(size_t)p * N + r] = sign ? sign * w : 0.5 + w;
            }
        return v;
    }
    // In constructRankStable's slot layout with no self offset (the self slot
    // is a tie like any other, groupAggregate), s_b the composite sign of
    // key_r - key_j and u_bc column c's value at row j in the same layout:
    //   v_b     = EvalTieTerm(s_b, W_b, 1/2),  W_b = -w_b     two levels below the sign
    //   g_b     = p_b + v_b,  p_b = 1/2 + w_b                 the 0/1 indicator "row j is in row r's frame"
    //   sum_cr  = fold(sum_b g_b (.) u_bc)_r                   one level below v
    //   count_r = K_r + fold(sum_b v_b)_r,  K_r = sum_d p      at v's level
    // The frames differ in w alone (windowWeight).  Per batch on its lane:
    // vecRotsOpt of the key and of every column (shared masks), the sign and
    // the tie term; after the join ONE EvalWeightSumMany for all batches and
    // columns and the rank's doubling folds, as groupAggregate.  Depth
    // windowDepth: the stable rank's plus the gated product; the count ends one
    // level above the sums.  Eager (no graph).  Preconditions: two keys are
    // equal or at least the sign configuration's resolution apart; payload
    // values lie in [-1, 1].
    WindowResult windowSums(const Ciphertext<DCRTPoly>& keys, const std::vector<Ciphertext<DCRTPoly>>& cols,
                            SignFunc SignFunc, SignConfig& Cfg, int frame, bool wantCount, size_t maxCols) {
        const size_t C = cols.size();
        if (frame != kFrameRows && frame != kFrameRange && frame != kFrameBelow)
            throw std::invalid_argument("window: unknown frame " + std::to_string(frame) +
                                        " (0 rows, 1 range, 2 below)");
        if (C > maxCols)
            throw std::invalid_argument("window: " + std::to_string(C) + " payload columns (at most " +
                                        std::to_string(maxCols) + ")");
        for (const auto& c : cols)
            if (c->GetLevel() != keys->GetLevel() || c->GetSlots() != keys->GetSlots())
                throw std::invalid_argument("window: the key and the columns must be at one level and slot count");
        const int need = (int)keys->GetLevel() + sfhe::windowDepth(Cfg.compos);
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("window: needs multiplicative depth " + std::to_string(need) +
                                   " (the stable rank's and one level for the gated product); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        const auto pre = rankBabyRotations(keys, L);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> preCols(C);
        for (size_t c = 0; c < C; ++c) preCols[c] = rankBabyRotations(cols[c], L);
        ph.mark("window: baby rotations");

        std::vector<Ciphertext<DCRTPoly>> v(L.B);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> u(C, std::vector<Ciphertext<DCRTPoly>>(L.B));
        const auto split = runBatches(L.B, [&](int b) {
            auto shifted = vecRotsOpt(pre, L.P, L.S, L.npRank, b);
            for (size_t c = 0; c < C; ++c) u[c][b] = vecRotsOpt(preCols[c], L.P, L.S, L.npRank, b);
            ph.mark("  window batch: vecRotsOpt");
            auto dup = keys->Clone();
            dup->SetSlots(L.S);
            auto s = sign(m_cc->EvalSub(dup, shifted), m_cc, SignFunc, Cfg);
            const Plaintext& W = memoPlain(kWindowWeights, frame, b, s->GetLevel(), L.S,
                                           [&] { return generateWindowWeights(L.S, L.P, b, frame, -1); });
            v[b] = m_cc->EvalTieTerm(s, W, 0.5);
            ph.mark("  window batch: sign + tie term");
        });
        split.gatherParts(m_cc, v);
        for (auto& col : u) split.gatherParts(m_cc, col);
        ph.mark("window: batches");

        auto fold = [&](Ciphertext<DCRTPoly> x) {
            x->SetSlots(L.S);
            return sumOverPartitions(x, {}, L.S);
        };
        WindowResult out;
        if (C) {
            std::vector<Plaintext> p(L.B);
            for (int b = 0; b < L.B; ++b)
                p[b] = memoPlain(kWindowGate, frame, b, v[b]->GetLevel(), L.S,
                                 [&] { return generateWindowWeights(L.S, L.P, b, frame, 0); });
            out.sums = m_cc->EvalWeightSumMany(v, p, u);
            for (auto& x : out.sums) x = fold(x);
        }
        ph.mark("window: weighted sums + folds");
        if (wantCount) {
            auto acc = v[0]->Clone();
            for (int b = 1; b < L.B; ++b) m_cc->EvalAddInPlace(acc, v[b]);
            acc = fold(acc);
            const Plaintext& K = memoPlain(kWindowCount, frame, 0, acc->GetLevel(), N, [&] {
                std::vector<double> k(N, 0.0);
                for (int r = 0; r < N; ++r)
                    for (int d = 0; d < N; ++d) k[r] += 0.5 + windowWeight(frame, r, d);
                return k;
            });
            out.count = m_cc->EvalAdd(acc, K);
        }
        ph.mark("window: count");
        return out;
    }

    // ---- join of two tables on up to SFHE_LEX_KEYS keys (SELECT a.*, COUNT(b.*),
    // SUM(b.col) FROM a LEFT JOIN b ON a.k1 = b.k1 AND ...) ----
    struct JoinResult {
        Ciphertext<DCRTPoly> count;              // count_r = #{j : keyB_kj = keyA_kr for every k}
        std::vector<Ciphertext<DCRTPoly>> sums;  // sums[c]_r = sum of colsB[c]_j over those j
    };
    // Every result is in table A's input order.  In groupAggregate's slot
    // layout (slot pN + r of batch b pairs A's row r with B's row j = (r + d)
    // mod N, d = bP + p; no self offset), with s_kb the composite sign of
    // keyA_kr - keyB_kj, q_kb = s_kb^2 ("key k differs"), Q_b = q_1b v ... v q_mb
    // ("some key differs": a balanced tree of m - 1 EvalGateOr, (q1 v q2) v q3
    // for m = 3) and u_bc column c of B at row j in the same layout:
    //   count_r  = N - fold(sum_b Q_b)_r                    at Q's level
    //   sum_cr   = fold(sum_b (1 - Q_b) (.) u_bc)_r          one level below Q
    // The flow is groupAggregate's: the baby rotations of B's keys and columns
    // (table A needs no rotation: its keys are only widened to S slots), each
    // batch on its lane, after the join ONE EvalGateSumMany for all batches and
    // columns, the sum of the Q_b and the rank's doubling folds.  With m = 1
    // and keysA[0], keysB[0] one ciphertext the op sequence is groupAggregate's
    // without the index.  Depth joinDepth: the grouping's plus ceil(log2 m);
    // the count ends one level above the sums.  Eager (no graph).
    // Preconditions: per key, any A value and any B value are equal or at
    // least the sign configuration's resolution apart, and their difference is
    // in the sign's domain (the keys are in the sort's input range); both
    // tables occupy N rows (a shorter B is padded with a key no A row takes,
    // A's padded rows are ignored by the client).
    // With unique B keys the count is the 0/1 semi-join flag (1 - count the
    // anti-join flag) and a sum is the looked-up value; a table joined with
    // itself on m keys is GROUP BY k1, ..., km.
    JoinResult joinAggregate(const std::vector<Ciphertext<DCRTPoly>>& keysA,
                             const std::vector<Ciphertext<DCRTPoly>>& keysB,
                             const std::vector<Ciphertext<DCRTPoly>>& colsB, SignFunc SignFunc, SignConfig& Cfg,
                             size_t maxCols) {
        const size_t m = keysA.size(), C = colsB.size();
        if (m < 1 || m > SFHE_LEX_KEYS)
            throw std::invalid_argument("join: " + std::to_string(m) + " keys (1 .. " +
                                        std::to_string(SFHE_LEX_KEYS) + ")");
        if (keysB.size() != m)
            throw std::invalid_argument("join: " + std::to_string(m) + " keys of table A against " +
                                        std::to_string(keysB.size()) + " of table B");
        if (C > maxCols)
            throw std::invalid_argument("join: " + std::to_string(C) + " payload columns (at most " +
                                        std::to_string(maxCols) + ")");
        const auto& k0 = keysA[0];
        for (const auto* list : {&keysA, &keysB, &colsB})
            for (const auto& c : *list)
                if (c->GetLevel() != k0->GetLevel() || c->GetSlots() != k0->GetSlots())
                    throw std::invalid_argument("join: the keys and the columns must be at one level and slot count");
        const int need = (int)k0->GetLevel() + sfhe::joinDepth(Cfg.compos, (int)m);
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("join: needs multiplicative depth " + std::to_string(need) +
                                   " (the grouping's and one level per layer of the keys' OR tree); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> pre(m), preCols(C);
        for (size_t k = 0; k < m; ++k) pre[k] = rankBabyRotations(keysB[k], L);
        for (size_t c = 0; c < C; ++c) preCols[c] = rankBabyRotations(colsB[c], L);
        ph.mark("join: baby rotations");

        // Q over q[lo, hi): the halves' ORs, the first half taking the odd key
        std::function<Ciphertext<DCRTPoly>(const std::vector<Ciphertext<DCRTPoly>>&, size_t, size_t)> orTree =
            [&](const std::vector<Ciphertext<DCRTPoly>>& q, size_t lo, size_t hi) {
                if (hi - lo == 1) return q[lo];
                const size_t mid = lo + (hi - lo + 1) / 2;
                return m_cc->EvalGateOr(orTree(q, lo, mid), orTree(q, mid, hi));
            };
        std::vector<Ciphertext<DCRTPoly>> Q(L.B);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> u(C, std::vector<Ciphertext<DCRTPoly>>(L.B));
        const auto split = runBatches(L.B, [&](int b) {
            std::vector<Ciphertext<DCRTPoly>> shifted(m), q(m);
            for (size_t k = 0; k < m; ++k) shifted[k] = vecRotsOpt(pre[k], L.P, L.S, L.npRank, b);
            for (size_t c = 0; c < C; ++c) u[c][b] = vecRotsOpt(preCols[c], L.P, L.S, L.npRank, b);
            ph.mark("  join batch: vecRotsOpt");
            for (size_t k = 0; k < m; ++k) {
                auto dup = keysA[k]->Clone();
                dup->SetSlots(L.S);
                auto s = sign(m_cc->EvalSub(dup, shifted[k]), m_cc, SignFunc, Cfg);
                q[k] = m_cc->EvalMult(s, s);
            }
            Q[b] = orTree(q, 0, m);
            ph.mark("  join batch: signs + gate");
        });
        split.gatherParts(m_cc, Q);
        for (auto& col : u) split.gatherParts(m_cc, col);
        ph.mark("join: batches");

        auto fold = [&](Ciphertext<DCRTPoly> x) {
            x->SetSlots(L.S);
            return sumOverPartitions(x, {}, L.S);
        };
        JoinResult out;
        if (C) {
            out.sums = m_cc->EvalGateSumMany(Q, u);
            for (auto& x : out.sums) x = fold(x);
        }
        ph.mark("join: gated sums + folds");
        auto acc = Q[0]->Clone();
        for (int b = 1; b < L.B; ++b) m_cc->EvalAddInPlace(acc, Q[b]);
        out.count = m_cc->EvalSub((double)N, fold(acc));
        ph.mark("join: count");
        return out;
    }

    // The masks of one baby/giant-step move and its giant steps' rotation amounts
    struct GiantMasks {
        std::vector<const std::vector<Plaintext>*> masks;  // [giant step][baby step]
        std::vector<int> steps;
    };
    // blindRotationOptN's: partition np*i + j kept, rotated by its baby step j
    GiantMasks blindRotationMasks(int num_slots, int np, uint32_t level) {
        std::vector<std::array<int, 5>> keys;
        GiantMasks gm;
        for (int i = 0; i < (num_slots / N) / np; ++i) {
            keys.push_back({kBlindMasks, 0, i, (int)level, num_slots});
            gm.steps.push_back(i * np);
        }
        gm.masks = maskMemoMany(keys, np, [&](size_t i, int j) {
            return m_cc->MakeCKKSPackedPlaintext(vectorRotate(generateMaskVectorN(num_slots, np * (int)i + j), j), 1,
                                                 level, nullptr, num_slots);
        });
        return gm;
    }

    // Rotates partition k = np*i + j of the masked inputs left by ib*P + k
    // (giant steps summed as in vecRotsOpt: one rotation by ib*P of a
    // rotateSum over i*np).
    Ciphertext<DCRTPoly> blindRotationOptN(const std::vector<Ciphertext<DCRTPoly>>& masked_inputs,
                                           int num_slots, int np, int ib, int num_partition) {
        const auto gm = blindRotationMasks(num_slots, np, masked_inputs[0]->GetLevel());
        std::vector<Ciphertext<DCRTPoly>> giants;
        for (const auto* m : gm.masks) giants.push_back(m_cc->EvalMultAddPlain(masked_inputs, *m));
        auto result = this->getZero()->Clone();
        m_cc->EvalAddInPlace(result, rot.rotate(rot.rotateSum(giants, gm.steps), ib * num_partition));
        return result;
    }
    // blindRotationOptN of several columns' masked inputs [c][j]: the columns
    // share the masks, so their giant-step sums are formed together
    // (EvalMultAddPlainCols); each column's sums then rotate as there.
    std::vector<Ciphertext<DCRTPoly>> blindRotationOptNCols(
        const std::vector<std::vector<Ciphertext<DCRTPoly>>>& masked_inputs, int num_slots, int np, int ib,
        int num_partition) {
        const auto gm = blindRotationMasks(num_slots, np, masked_inputs[0][0]->GetLevel());
        const auto giants = m_cc->EvalMultAddPlainCols(masked_inputs, gm.masks);
        std::vector<Ciphertext<DCRTPoly>> results;
        for (const auto& g : giants) {
            auto result = this->getZero()->Clone();
            m_cc->EvalAddInPlace(result, rot.rotate(rot.rotateSum(g, gm.steps), ib * num_partition));
            results.push_back(result);
        }
        return results;
    }

    // index - rank at S slots: what both placements compare with their
    // batches' checking vectors
    Ciphertext<DCRTPoly> indexMinusRank(const Ciphertext<DCRTPoly>& ctx_Rank, const sfhe::RankLayout& L) {
        auto d = m_cc->EvalSub(indexPlain(ctx_Rank->GetLevel()), ctx_Rank);
        d->SetSlots(L.S);
        return d;
    }

    Ciphertext<DCRTPoly> rotationIndexCheckN(const Ciphertext<DCRTPoly>& ctx_Rank,
                                             const Ciphertext<DCRTPoly>& input_array) {
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        auto output = this->getZero()->Clone();
        const auto offset = indexMinusRank(ctx_Rank, L);
        input_array->SetSlots(L.S);  // reference side effect (sort_algo.h:711)
        const sfhe::SincIndicator ind(N);
        std::vector<Ciphertext<DCRTPoly>> parts(L.B);
        const auto split = runBatches(L.B, [&](int b) {
            // (r - rank_r - c) / 2N  in (-1, 1/2)
            auto hit = ind.hit(m_cc, m_cc->EvalSub(offset, checkingPlain(b, offset->GetLevel(), L)), ph);
            auto masked = m_cc->EvalMult(hit, input_array);
            auto maskedRot = rot.rotateMany(masked, babySteps(L.npPlace));
            ph.mark("  place batch: mask + baby rotations");
            parts[b] = blindRotationOptN(maskedRot, L.S, L.npPlace, b, L.P);
            ph.mark("  place batch: blind rotation");
        });
        split.gatherParts(m_cc, parts);
        output = sumOverPartitions(output, parts, L.S);
        ph.mark("place: batch sum + folds");
        return output;
    }

    // The placement of several columns by ONE rank (records: a key and its
    // payload columns).  The indicator `hit` depends on the
    // rank alone: per batch it is evaluated once, exactly as in
    // rotationIndexCheckN, and only the linear tail (hit (.) column, baby
    // rotations, blind rotation, batch sum, folds) runs per column.  Column c
    // of the result holds the residues of rotationIndexCheckN(ctx_Rank,
    // cols[c]): the arithmetic is exact on canonical residues, so sharing
    // `hit` changes none of them.  Every column is left at S slots, as
    // rotationIndexCheckN leaves its input.
    std::vector<Ciphertext<DCRTPoly>> placeMany(const Ciphertext<DCRTPoly>& ctx_Rank,
                                                const std::vector<Ciphertext<DCRTPoly>>& cols) {
        if (cols.empty()) throw OpenFHEException("placeMany: no columns");
        for (const auto& c : cols)
            if (c->GetLevel() != cols[0]->GetLevel())
                throw OpenFHEException("placeMany: the columns must be at one level");
        const sfhe::RankLayout L(N, max_batch);
        sfhe::PhaseTimer ph(m_cc);
        const size_t C = cols.size();
        const auto offset = indexMinusRank(ctx_Rank, L);
        for (const auto& c : cols) c->SetSlots(L.S);  // (rotationIndexCheckN's side effect on its input)
        const sfhe::SincIndicator ind(N);
        std::vector<std::vector<Ciphertext<DCRTPoly>>> parts(C, std::vector<Ciphertext<DCRTPoly>>(L.B));
        const auto split = runBatches(L.B, [&](int b) {
            auto hit = ind.hit(m_cc, m_cc->EvalSub(offset, checkingPlain(b, offset->GetLevel(), L)), ph);
            std::vector<std::vector<Ciphertext<DCRTPoly>>> maskedRot(C);
            for (size_t c = 0; c < C; ++c)
                maskedRot[c] = rot.rotateMany(m_cc->EvalMult(hit, cols[c]), babySteps(L.npPlace));
            ph.mark("  place batch: masks + baby rotations");
            auto placed = blindRotationOptNCols(maskedRot, L.S, L.npPlace, b, L.P);
            for (size_t c = 0; c < C; ++c) parts[c][b] = placed[c];
            ph.mark("  place batch: blind rotations");
        });
        m_cc->NotePlacement(split.mine.size(), C);
        std::vector<Ciphertext<DCRTPoly>> outputs(C);
        for (size_t c = 0; c < C; ++c) {
            split.gatherParts(m_cc, parts[c]);
            outputs[c] = sumOverPartitions(this->getZero()->Clone(), parts[c], L.S);
        }
        ph.mark("place: batch sums + folds");
        return outputs;
    }

    // ---- selection by rank: order statistics without the
    // full placement.  rotationIndexCheckN is offset-major -- slot pN + r of
    // batch b asks "does element r move left by bP + p?" -- so every one of
    // its B = N/P batches (a doubled-sinc PS each) feeds every output.  Here
    // the layout is target-major: partition p of batch b asks "which element
    // has rank t = targets[b Psel + p]?", K targets take ceil(K / Psel)
    // batches, Psel = min(nextpow2(K), P) partitions of N slots:
    //   hit[pN + r] = D(((t - rank_r) zmul/2N) + zadd), t - rank_r in (-N, N):
    //                 only the hit at 0 can occur (the same rebased doubled
    //                 sinc, PS and level adjustment as the placement);
    //   masked = hit (.) input; its N slots of a partition are summed into
    //   slot pN by radix-4 EvalRotateFold steps (strides 1, 4, 16, ..., a
    //   last step of 2 terms where log2 N is odd);
    //   one plaintext mask keeps slot pN of the real targets -- the level
    //   `place` spends on its masks -- inside the baby/giant-step move of that
    //   slot to a slot congruent to c = b Psel + p modulo N: a left rotation
    //   by N - c = base_b + p', p' = Psel - 1 - p = np i + j, base_b =
    //   N + 1 - (b + 1) Psel (baby steps j, giant steps np i, then base_b);
    //   the batches are summed and the folds S/2 .. N make the sum N-periodic.
    // Slot i < K of the result holds the element of rank targets[i], the
    // other slots 0 up to noise; the level is the one `place` leaves.  Runs
    // eagerly (no graph).  The masks depend on the target list, which is
    // part of their memo key (an id per distinct list, kept for the sorter's
    // lifetime: a caller cycling through many lists grows the memo).
    std::map<std::vector<int>, int> m_targetIds;
    int targetListId(const std::vector<int>& targets) {
        std::lock_guard<std::mutex> g(m_masksMu);
        auto it = m_targetIds.find(targets);
        if (it != m_targetIds.end()) return it->second;
        const int id = (int)m_targetIds.size();
        return m_targetIds[targets] = id;
    }

    // sum of the N slots of every partition into its first slot
    Ciphertext<DCRTPoly> foldPartitions(Ciphertext<DCRTPoly> x) {
        int stride = 1;
        for (; stride * 4 <= N; stride *= 4) x = m_cc->EvalRotateFold(x, stride, 4);
        if (stride < N) x = m_cc->EvalRotateFold(x, stride, 2);
        return x;
    }

    // the checks every selection runs first: the target list, and the depth a rank at this level needs
    void selectCheck(const Ciphertext<DCRTPoly>& ctx_Rank, const std::vector<int>& targets,
                     const sfhe::SincIndicator& ind) {
        const int K = (int)targets.size();
        if (K < 1 || K > N) throw std::invalid_argument("select: the target count must be in [1, N]");
        {
            std::vector<char> seen(N, 0);
            for (int t : targets) {
                if (t < 0 || t >= N) throw std::invalid_argument("select: target rank " + std::to_string(t) +
                                                                 " is outside [0, N)");
                if (seen[t]) throw std::invalid_argument("select: duplicate target rank " + std::to_string(t));
                seen[t] = 1;
            }
        }
        const int need = (int)ctx_Rank->GetLevel() + 1 + (int)ind.psDepth + 1 + 1;
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("select: needs multiplicative depth " + std::to_string(need) +
                                   " from a rank at level " + std::to_string(ctx_Rank->GetLevel()) +
                                   "; the context has " + std::to_string(m_cc->GetMultiplicativeDepth()));
    }

    // The target-major layout of a selection of K = targets.size() ranks, and
    // the target list's memo id.
    struct SelectLayout {
        int K, Psel, S, B, np, tid;
    };
    SelectLayout selectLayout(const std::vector<int>& targets) {
        const sfhe::RankLayout L(N, max_batch);
        SelectLayout sel;
        sel.K = (int)targets.size();
        sel.Psel = 1;
        while (sel.Psel < sel.K && sel.Psel < L.P) sel.Psel *= 2;
        sel.S = N * sel.Psel;
        sel.B = (sel.K + sel.Psel - 1) / sel.Psel;
        sel.np = 1 << (sfhe::ilog2(sel.Psel) / 2);
        sel.tid = targetListId(targets);
        return sel;
    }
    // T[pN + r] = targets[b Psel + p] (a padded partition repeats the batch's first target)
    const Plaintext& targetPlain(const SelectLayout& sel, const std::vector<int>& targets, int b, uint32_t level) {
        return memoPlain(kTargets, b, sel.tid, level, sel.S, [&] {
            std::vector<double> T(sel.S);
            for (int p = 0; p < sel.Psel; ++p) {
                const int k = b * sel.Psel + p;
                std::fill(T.begin() + (size_t)p * N, T.begin() + (size_t)(p + 1) * N,
                          (double)targets[k < sel.K ? k : b * sel.Psel]);
            }
            return T;
        });
    }
    // The move of batch b: slot pN of the real targets kept, inside baby steps
    // j and giant steps np g (p' = Psel - 1 - p = np g + j); base_b follows.
    GiantMasks moveMasks(const SelectLayout& sel, int b, uint32_t level) {
        std::vector<std::array<int, 5>> keys;
        GiantMasks gm;
        for (int g = 0; g < sel.Psel / sel.np; ++g) {
            keys.push_back({kMoveMasks, sel.tid, b * 1024 + g, (int)level, sel.S});
            gm.steps.push_back(g * sel.np);
        }
        gm.masks = maskMemoMany(keys, sel.np, [&](size_t g, int j) {
            std::vector<double> m(sel.S, 0.0);
            const int p = sel.Psel - 1 - (sel.np * (int)g + j);
            if (b * sel.Psel + p < sel.K) m[(size_t)p * N] = 1.0;
            return m_cc->MakeCKKSPackedPlaintext(vectorRotate(m, j), 1, level, nullptr, sel.S);
        });
        return gm;
    }
    int moveBase(const SelectLayout& sel, int b) const { return (N + 1 - (b + 1) * sel.Psel) % sel.S; }

    Ciphertext<DCRTPoly> selectRanks(const Ciphertext<DCRTPoly>& ctx_Rank, const Ciphertext<DCRTPoly>& input_array,
                                     const std::vector<int>& targets) {
        const sfhe::SincIndicator ind(N);
        selectCheck(ctx_Rank, targets, ind);
        const auto sel = selectLayout(targets);
        sfhe::PhaseTimer ph(m_cc);
        auto rankS = ctx_Rank->Clone();
        rankS->SetSlots(sel.S);
        auto input = input_array->Clone();
        input->SetSlots(sel.S);
        std::vector<Ciphertext<DCRTPoly>> parts(sel.B);
        const auto split = runBatches(sel.B, [&](int b) {
            // (t - rank_r) / 2N  in (-1/2, 1/2)
            auto hit = ind.hit(m_cc, m_cc->EvalSub(targetPlain(sel, targets, b, rankS->GetLevel()), rankS), ph);
            auto summed = foldPartitions(m_cc->EvalMult(hit, input));
            ph.mark("  select batch: mask + in-partition folds");
            auto pre = rot.rotateMany(summed, babySteps(sel.np));
            const auto gm = moveMasks(sel, b, pre[0]->GetLevel());
            std::vector<Ciphertext<DCRTPoly>> giants;
            for (const auto* m : gm.masks) {
                giants.push_back(m_cc->EvalMultAddPlain(pre, *m));
                giants.back()->SetSlots(sel.S);
            }
            parts[b] = rot.rotate(rot.rotateSum(giants, gm.steps), moveBase(sel, b));
            ph.mark("  select batch: move");
        });
        m_cc->NoteSelection(split.mine.size());
        split.gatherParts(m_cc, parts);
        auto output = this->getZero()->Clone();
        output->SetSlots(sel.S);
        output = sumOverPartitions(output, parts, sel.S);
        ph.mark("select: batch sum + folds");
        return output;
    }

    // The (stable) rank of `input_array`, then selectRanks of its own values.
    Ciphertext<DCRTPoly> select(const Ciphertext<DCRTPoly>& input_array, const std::vector<int>& targets,
                                SignFunc SignFunc, SignConfig& Cfg, bool stable) {
        auto rank = stable ? constructRankStable(input_array, SignFunc, Cfg) : constructRank(input_array, SignFunc, Cfg);
        return selectRanks(rank, input_array, targets);
    }

    // foldPartitions of several columns of one level (EvalRotateFoldMany per step)
    std::vector<Ciphertext<DCRTPoly>> foldPartitionsMany(std::vector<Ciphertext<DCRTPoly>> x) {
        int stride = 1;
        for (; stride * 4 <= N; stride *= 4) x = m_cc->EvalRotateFoldMany(x, stride, 4);
        if (stride < N) x = m_cc->EvalRotateFoldMany(x, stride, 2);
        return x;
    }

    // The selection of several columns by ONE rank (ORDER BY key LIMIT k over
    // rows).  As in placeMany the indicator depends on the rank
    // and the target list alone: per batch it is evaluated once, exactly as in
    // selectRanks (the same target plaintexts and move masks, no memo entries
    // of its own), and the linear tail runs per column -- the in-partition
    // folds of all columns by EvalRotateFoldMany, the move's giant-step sums by
    // EvalMultAddPlainCols (shared masks).  Column c of the result holds the
    // residues of selectRanks(ctx_Rank, cols[c], targets).
    std::vector<Ciphertext<DCRTPoly>> selectRanksMany(const Ciphertext<DCRTPoly>& ctx_Rank,
                                                      const std::vector<Ciphertext<DCRTPoly>>& cols,
                                                      const std::vector<int>& targets) {
        if (cols.empty()) throw OpenFHEException("selectRanksMany: no columns");
        for (const auto& c : cols)
            if (c->GetLevel() != cols[0]->GetLevel())
                throw OpenFHEException("selectRanksMany: the columns must be at one level");
        const sfhe::SincIndicator ind(N);
        selectCheck(ctx_Rank, targets, ind);
        const auto sel = selectLayout(targets);
        const size_t C = cols.size();
        sfhe::PhaseTimer ph(m_cc);
        auto rankS = ctx_Rank->Clone();
        rankS->SetSlots(sel.S);
        std::vector<Ciphertext<DCRTPoly>> inputs(C);
        for (size_t c = 0; c < C; ++c) {
            inputs[c] = cols[c]->Clone();
            inputs[c]->SetSlots(sel.S);
        }
        std::vector<std::vector<Ciphertext<DCRTPoly>>> parts(C, std::vector<Ciphertext<DCRTPoly>>(sel.B));
        const auto split = runBatches(sel.B, [&](int b) {
            auto hit = ind.hit(m_cc, m_cc->EvalSub(targetPlain(sel, targets, b, rankS->GetLevel()), rankS), ph);
            std::vector<Ciphertext<DCRTPoly>> masked(C);
            for (size_t c = 0; c < C; ++c) masked[c] = m_cc->EvalMult(hit, inputs[c]);
            const auto summed = foldPartitionsMany(masked);
            ph.mark("  select batch: masks + in-partition folds");
            std::vector<std::vector<Ciphertext<DCRTPoly>>> pre(C);
            for (size_t c = 0; c < C; ++c) pre[c] = rot.rotateMany(summed[c], babySteps(sel.np));
            const auto gm = moveMasks(sel, b, pre[0][0]->GetLevel());
            const auto giants = m_cc->EvalMultAddPlainCols(pre, gm.masks);
            for (size_t c = 0; c < C; ++c) {
                for (const auto& gct : giants[c]) gct->SetSlots(sel.S);
                parts[c][b] = rot.rotate(rot.rotateSum(giants[c], gm.steps), moveBase(sel, b));
            }
            ph.mark("  select batch: moves");
        });
        m_cc->NoteSelection(split.mine.size());
        m_cc->NoteSelectionColumns(C);
        std::vector<Ciphertext<DCRTPoly>> outputs(C);
        for (size_t c = 0; c < C; ++c) {
            split.gatherParts(m_cc, parts[c]);
            auto output = this->getZero()->Clone();
            output->SetSlots(sel.S);
            outputs[c] = sumOverPartitions(output, parts[c], sel.S);
        }
        ph.mark("select: batch sums + folds");
        return outputs;
    }

    // ORDER BY key LIMIT k over rows: the (stable) rank of `keys`, then
    // selectRanksMany of {keys, cols...}: first the selected keys, then the
    // selected columns.
    std::vector<Ciphertext<DCRTPoly>> selectRecords(const Ciphertext<DCRTPoly>& keys,
                                                    const std::vector<Ciphertext<DCRTPoly>>& cols,
                                                    const std::vector<int>& targets, SignFunc SignFunc,
                                                    SignConfig& Cfg, bool stable) {
        auto rank = stable ? constructRankStable(keys, SignFunc, Cfg) : constructRank(keys, SignFunc, Cfg);
        std::vector<Ciphertext<DCRTPoly>> in{keys};
        in.insert(in.end(), cols.begin(), cols.end());
        return selectRanksMany(rank, in, targets);
    }

    // ---- records ordered by several keys (ORDER BY a, b [DESC]) ----
    // The keys and payload columns of a lexicographic record sort / selection:
    // {keys..., cols...}, as many columns as a one-key record call takes.
    std::vector<Ciphertext<DCRTPoly>> lexColumns(const char* what, const std::vector<Ciphertext<DCRTPoly>>& keys,
                                                 const std::vector<Ciphertext<DCRTPoly>>& cols, size_t maxCols) {
        if (keys.size() + cols.size() > 1 + maxCols)
            throw OpenFHEException(std::string(what) + ": " + std::to_string(keys.size()) + " keys and " +
                                   std::to_string(cols.size()) + " payload columns (at most " +
                                   std::to_string(1 + maxCols) + " columns in all)");
        std::vector<Ciphertext<DCRTPoly>> in(keys);
        in.insert(in.end(), cols.begin(), cols.end());
        return in;
    }
    void lexDepthCheck(const char* what, const std::vector<Ciphertext<DCRTPoly>>& keys, SignConfig& Cfg) {
        if (keys.empty()) return;  // (constructRankLex refuses)
        const int need = (int)keys[0]->GetLevel() + sfhe::lexSortDepth(N, Cfg.compos, (int)keys.size());
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException(std::string(what) + ": needs multiplicative depth " + std::to_string(need) +
                                   " (the stable sort's, and one level per key after the first); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
    }
    // constructRankLex + ONE placement of {keys..., cols...} (placeMany): the
    // sorted keys in their order, then the sorted columns.  Eager (no graph
    // cache: the record sort's eager and captured times are equal, §4f).
    std::vector<Ciphertext<DCRTPoly>> sortRecordsLex(const std::vector<Ciphertext<DCRTPoly>>& keys,
                                                     const std::vector<Ciphertext<DCRTPoly>>& cols,
                                                     const std::vector<bool>& descending, SignFunc SignFunc,
                                                     SignConfig& Cfg, size_t maxCols) {
        const auto in = lexColumns("lexicographic record sort", keys, cols, maxCols);
        lexDepthCheck("lexicographic record sort", keys, Cfg);
        return placeMany(constructRankLex(keys, descending, SignFunc, Cfg), in);
    }
    // constructRankLex + selectRanksMany of {keys..., cols...} (eager, §4g)
    std::vector<Ciphertext<DCRTPoly>> selectRecordsLex(const std::vector<Ciphertext<DCRTPoly>>& keys,
                                                       const std::vector<Ciphertext<DCRTPoly>>& cols,
                                                       const std::vector<int>& targets,
                                                       const std::vector<bool>& descending, SignFunc SignFunc,
                                                       SignConfig& Cfg, size_t maxCols) {
        const auto in = lexColumns("lexicographic record selection", keys, cols, maxCols);
        return selectRanksMany(constructRankLex(keys, descending, SignFunc, Cfg), in, targets);
    }

    // ---- hybrid placement I (reference :815-891,
    // :1067-1229).  Rank as DirectSort; placement by an indicator matrix:
    // with M = min(N, 256) and num_slots = M*M per batch, slot (i, j) of
    // batch b holds indicator(b*M + i - rank_{(j + k M) mod N}) * x_{(j + k M) mod N}
    // summed over the rank rotations k; the row sums land in column b
    // (sumColumnsToTarget) and that column becomes row b (transposeColumnTarget),
    // so the first N slots of the sum over batches hold the sorted array.
    std::vector<bool> getBinaryPath(size_t columnIndex, size_t matrixSize) {
        const size_t bits = LOG2(matrixSize);
        std::vector<bool> path(bits);
        for (size_t i = 0; i < bits; ++i) path[i] = (columnIndex >> (bits - 1 - i)) & 1;
        return path;
    }

    // sums the matrixSize entries of every row into column columnIndex (a
    // binary tree of rotations by +-matrixSize/2, ..., 1: left child on 0,
    // right child on 1), optionally masking everything else out
    Ciphertext<DCRTPoly> sumColumnsToTarget(Ciphertext<DCRTPoly> c, const size_t matrixSize,
                                            const size_t columnIndex, bool maskOutput) {
        const auto path = getBinaryPath(columnIndex, matrixSize);
        size_t step = matrixSize >> 1;
        c->SetSlots((uint32_t)(matrixSize * matrixSize));
        for (size_t i = 0; i < path.size(); ++i, step >>= 1)
            c = m_cc->EvalAdd(c, rot.rotate(c, path[i] ? -(int)step : (int)step));
        if (maskOutput) {
            const Plaintext& pmsk = maskMemo({kColumnMask, (int)matrixSize, (int)columnIndex, (int)c->GetLevel(), 0},
                                             [&](auto& v) {
                                                 std::vector<double> msk(matrixSize * matrixSize, 0.0);
                                                 for (size_t i = 0; i < matrixSize; ++i)
                                                     msk[matrixSize * i + columnIndex] = 1.0;
                                                 v.push_back(m_cc->MakeCKKSPackedPlaintext(
                                                     msk, 1, c->GetLevel(), nullptr,
                                                     (uint32_t)(matrixSize * matrixSize)));
                                             })[0];
            c = m_cc->EvalMult(c, pmsk);
        }
        return c;
    }

    // moves column rowIndex to row rowIndex: rotations by
    // +-M(M-1)/2, +-M(M-1)/4, ..., the path of rowIndex choosing the sign
    Ciphertext<DCRTPoly> transposeColumnTarget(Ciphertext<DCRTPoly> c, const size_t matrixSize,
                                               const size_t rowIndex, bool maskOutput) {
        const auto path = getBinaryPath(rowIndex, matrixSize);
        size_t step = matrixSize * (matrixSize - 1) / 2;
        c->SetSlots((uint32_t)(matrixSize * matrixSize));
        for (size_t i = 0; i < path.size(); ++i, step >>= 1)
            c = m_cc->EvalAdd(c, rot.rotate(c, path[i] ? -(int)step : (int)step));
        if (maskOutput) {
            const Plaintext& pmsk = maskMemo({kRowMask, (int)matrixSize, (int)rowIndex, (int)c->GetLevel(), 0},
                                             [&](auto& v) {
                                                 std::vector<double> msk(matrixSize * matrixSize, 0.0);
                                                 for (size_t i = 0; i < matrixSize; ++i)
                                                     msk[matrixSize * rowIndex + i] = 1.0;
                                                 v.push_back(m_cc->MakeCKKSPackedPlaintext(
                                                     msk, 1, c->GetLevel(), nullptr,
                                                     (uint32_t)(matrixSize * matrixSize)));
                                             })[0];
            c = m_cc->EvalMult(c, pmsk);
        }
        return c;
    }

    // The MEHP24 matrix placement shared by the three hybrid sorts (reference
    // :894-1062 hybrid, :1067-1229 hybrid1, :1233-1389 hybrid2): with
    // M = min(N, 256) and num_slots = M*M per batch (the whole ring above 256),
    // slot (i, j) of batch b holds ind(sub_b(i) - rank_{(j + kM) mod N}) *
    // x_{(j + kM) mod N} summed over the rank rotations k; the row sums land
    // in column b (sumColumnsToTarget), that column becomes row b
    // (transposeColumnTarget), and the sum over batches holds the sorted array
    // in its first N slots.  `rank` is the (possibly 1/N-scaled) rank,
    // sub_b(i) = subScale (b M + i), `ind` the indicator of each variant.
    template <class Ind>
    Ciphertext<DCRTPoly> matrixPlacement(const Ciphertext<DCRTPoly>& rank, const Ciphertext<DCRTPoly>& input_array,
                                         double subScale, int memoTag, Ind&& ind) {
        constexpr size_t maxArraySize = 256;
        const size_t num_slots = N > (int)maxArraySize ? (size_t)max_batch : (size_t)N * N;
        const size_t num_batch = N > (int)maxArraySize ? N / maxArraySize : 1;
        const size_t M = std::min((size_t)N, maxArraySize);
        if (num_slots > (size_t)max_batch || M * M > num_slots)
            throw OpenFHEException("hybrid sort: N*N slots exceed the ring (needs ring dimension >= 2 N^2)");
        rank->SetSlots((uint32_t)num_slots);
        input_array->SetSlots((uint32_t)num_slots);
        std::vector<Ciphertext<DCRTPoly>> rots_Rank(num_batch), rots_Input(num_batch);
        for (size_t k = 0; k < num_batch; ++k) {
            rots_Rank[k] = rot.rotate(rank, (int)(k * maxArraySize));
            rots_Input[k] = rot.rotate(input_array, (int)(k * maxArraySize));
        }
        std::vector<Ciphertext<DCRTPoly>> Masked(num_batch);
        const int lanes = std::min((int)num_batch, m_cc->LaneCount());
        m_cc->ForkLanes(lanes, sfhe::stackBatches());
        sfhe::parallelLanes(m_cc, lanes, (int)num_batch, [&](int bi) {
            const size_t b = (size_t)bi;
            // subMask_b[i M + j] = subScale (b M + i) (reference :1089-1098, :929-939)
            const Plaintext& subMask =
                maskMemo({memoTag, bi, 0, (int)rank->GetLevel(), (int)num_slots}, [&](auto& v) {
                    std::vector<double> m(num_slots, 0.0);
                    for (size_t i = 0; i < M; ++i)
                        for (size_t j = 0; j < M; ++j) m[i * M + j] = subScale * (double)(b * M + i);
                    v.push_back(m_cc->MakeCKKSPackedPlaintext(m, 1, rank->GetLevel(), nullptr, (uint32_t)num_slots));
                })[0];
            auto subMasked = this->getZero()->Clone();
            subMasked->SetSlots((uint32_t)num_slots);
            for (size_t k = 0; k < num_batch; ++k) {
                auto rotationMask = ind(m_cc->EvalSub(subMask, rots_Rank[k]));
                subMasked = m_cc->EvalAdd(subMasked, m_cc->EvalMult(rots_Input[k], rotationMask));
            }
            subMasked = sumColumnsToTarget(subMasked, N / num_batch, b, true);
            Masked[b] = transposeColumnTarget(subMasked, N / num_batch, b, true);
        });
        m_cc->JoinLanes();
        return m_cc->EvalAddMany(Masked);
    }

    // hybrid I: MEHP24 indicatorAdv on the unscaled rank (reference :1067-1229)
    Ciphertext<DCRTPoly> rotationIndexCheckHybrid1(const Ciphertext<DCRTPoly>& ctx_Rank,
                                                   const Ciphertext<DCRTPoly>& input_array,
                                                   PrivateKey<DCRTPoly> sk) {
        (void)sk;  // (unused by the reference as well)
        // dg_i = (log2 N + 1) / 2 truncated (reference :1126-1127)
        const uint32_t dg_i = (uint32_t)((std::log2((double)N) + 1) / 2);
        const uint32_t df_i = 2;
        return matrixPlacement(ctx_Rank, input_array, 1.0, kHybrid1Sub, [&](const Ciphertext<DCRTPoly>& c) {
            return mehp24::utils::indicatorAdv(c, (double)N, dg_i, df_i);
        });
    }

    Ciphertext<DCRTPoly> sort_hybrid1(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                      SignConfig& Cfg, PrivateKey<DCRTPoly> sk) {
        auto ctx_Rank = constructRank(input_array, SignFunc, Cfg);
        return rotationIndexCheckHybrid1(ctx_Rank, input_array, sk);
    }

    // hybrid: rank / N against (b M + i) / N; the scaled-sinc Chebyshev series
    // below N = 256, the composite-sign indicator |d| < 1/2N at and above
    // (CompositeSign(3,4,2) at 256, (3,5,2) beyond; reference :894-1062)
    Ciphertext<DCRTPoly> rotationIndexCheckHybrid(const Ciphertext<DCRTPoly>& ctx_Rank,
                                                  const Ciphertext<DCRTPoly>& input_array,
                                                  PrivateKey<DCRTPoly> sk) {
        (void)sk;
        ctx_Rank->SetSlots(N > 256 ? (uint32_t)max_batch : (uint32_t)(N * N));
        auto r = m_cc->EvalMult(ctx_Rank, 1.0 / N);
        return matrixPlacement(r, input_array, 1.0 / N, kHybridSub, [&](const Ciphertext<DCRTPoly>& c) {
            if (N < 256) return m_cc->EvalChebyshevSeriesPS(c, selectCoefficients<N>(), -1, 1);
            SignConfig icfg(CompositeSignConfig(3, N < 512 ? 4 : 5, 2));
            return comp.indicator(m_cc, c, 0.5 / N, SignFunc::CompositeSign, icfg);
        });
    }

    Ciphertext<DCRTPoly> sort_hybrid(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                     SignConfig& Cfg, PrivateKey<DCRTPoly> sk) {
        auto ctx_Rank = constructRank(input_array, SignFunc, Cfg);
        return rotationIndexCheckHybrid(ctx_Rank, input_array, sk);
    }

    // hybrid II: the scaled-sinc series at every N (reference :1233-1389)
    Ciphertext<DCRTPoly> rotationIndexCheckHybrid2(const Ciphertext<DCRTPoly>& ctx_Rank,
                                                   const Ciphertext<DCRTPoly>& input_array,
                                                   PrivateKey<DCRTPoly> sk) {
        (void)sk;
        ctx_Rank->SetSlots(N > 256 ? (uint32_t)max_batch : (uint32_t)(N * N));
        auto r = m_cc->EvalMult(ctx_Rank, 1.0 / N);
        return matrixPlacement(r, input_array, 1.0 / N, kHybridSub, [&](const Ciphertext<DCRTPoly>& c) {
            return m_cc->EvalChebyshevSeriesPS(c, selectCoefficients<N>(), -1, 1);
        });
    }

    Ciphertext<DCRTPoly> sort_hybrid2(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                      SignConfig& Cfg, PrivateKey<DCRTPoly> sk) {
        auto ctx_Rank = constructRank(input_array, SignFunc, Cfg);
        return rotationIndexCheckHybrid2(ctx_Rank, input_array, sk);
    }

    // Placement over 2N-slot blocks with the scaled sinc (reference :537-656;
    // not called by the reference's sorts): P = min(2N, n/2/N) partitions of N
    // slots, B = 2N/P batches; batch b checks i - rank_i against the
    // 2N-periodic checking vector and rotates each N-slot block left by its
    // offset (blindRotationOpt2N).
    Ciphertext<DCRTPoly> blindRotationOpt2N(const std::vector<Ciphertext<DCRTPoly>>& masked_inputs, int num_slots,
                                            int np, int ib) {
        (void)ib;
        std::vector<Ciphertext<DCRTPoly>> giants;
        std::vector<int> steps;
        for (int i = 0; i < (num_slots / N / 2) / np; ++i) {
            auto& masks = maskMemo({kBlindMasks2N, 0, i, (int)masked_inputs[0]->GetLevel(), num_slots}, [&](auto& v) {
                for (int j = 0; j < np; ++j)
                    v.push_back(m_cc->MakeCKKSPackedPlaintext(vectorRotate(generateMaskVector2N(num_slots, np * i + j), j),
                                                              1, masked_inputs[j]->GetLevel(), nullptr, num_slots));
            });
            giants.push_back(m_cc->EvalMultAddPlain(masked_inputs, masks));
            steps.push_back(i * np);
        }
        auto result = this->getZero()->Clone();
        m_cc->EvalAddInPlace(result, rot.rotateSum(giants, steps));
        return result;
    }

    Ciphertext<DCRTPoly> rotationIndexCheck2N(const Ciphertext<DCRTPoly>& ctx_Rank,
                                              const Ciphertext<DCRTPoly>& input_array) {
        const int num_partition = std::min(2 * N, max_batch / N);
        const int num_batch = 2 * N / num_partition;
        const int num_slots = num_partition * N;
        // np = 2^floor(log2(num_partition / 2) / 2), halved while np^2 > num_partition / 2 (:597-600)
        int np = 1 << (sfhe::ilog2(num_partition / 2) >> 1);
        if (np * np > num_partition / 2) np >>= 1;
        auto output = this->getZero()->Clone();
        auto indexMinusRank = m_cc->EvalSub(indexPlain(ctx_Rank->GetLevel()), ctx_Rank);
        indexMinusRank->SetSlots(num_slots);
        input_array->SetSlots(num_slots);
        const int off = num_slots / N / 2;
        for (int b = 0; b < num_batch; ++b) {
            const Plaintext& chk = memoPlain(kCheckingVector2N, b, 0, indexMinusRank->GetLevel(), num_slots,
                                             [&] { return generateCheckingVector2N(num_slots, b * off); });
            // sinc on (i - rank - c) / 2N in (-1, 1)
            auto z = m_cc->EvalMult(m_cc->EvalSub(indexMinusRank, chk), 1.0 / N / 2);
            auto hit = m_cc->EvalChebyshevSeriesPS(z, selectCoefficients<N>(), -1, 1);
            auto masked = m_cc->EvalMult(hit, input_array);
            std::vector<Ciphertext<DCRTPoly>> masked_inputs(np);
            for (int i = 0; i < np; ++i) masked_inputs[i] = rot.rotate(masked, b * off + i);
            m_cc->EvalAddInPlace(output, blindRotationOpt2N(masked_inputs, num_slots, np, b));
        }
        for (int s = num_slots / 2; s >= num_slots / num_partition; s /= 2)
            m_cc->EvalAddInPlace(output, rot.rotate(output, s));
        output->SetSlots(N);
        return output;
    }

    // ---- hipGraph replay (north_star: "the Chebyshev tree / rotations /
    // rank-matrix EvalMults run as a hipGraph") ----
    // The op sequence of sort() depends only on (N, the input's level and
    // slots, the sign configuration), never on the data (reference
    // sort_algo.h:752-774).  The first sort of a shape runs eagerly (it
    // generates and encodes the masks); the second is captured into a graph
    // over a sorter-owned copy of the input; from then on a sort is: copy the
    // caller's input into that buffer, launch the graph, clone its result.
    // Debug sorts (PRINT_PT decrypts) replay two graphs with the decrypts
    // between them (sortDebug); contexts sharded over a host transport run
    // eagerly (BeginCapture refuses them); RCCL-sharded sorts capture their
    // collectives into the graph.  SFHE_GRAPH=0 disables graphs.
    struct GraphKey {
        uint32_t level = 0, slots = 0;
        int func = -1, n = 0, dg = 0, df = 0;
        int multDepth = 0;  // decides whether compositeSign records bootstraps
        bool stable = false;
        std::vector<std::pair<uint32_t, uint32_t>> cols;  // records: each payload column's (level, slots)
        bool operator==(const GraphKey& o) const {
            return level == o.level && slots == o.slots && func == o.func && n == o.n && dg == o.dg && df == o.df &&
                   multDepth == o.multDepth && stable == o.stable && cols == o.cols;
        }
    };
    // The key of a sort of `first` (the input, or the records' key column) and
    // the payload columns `cols`.  sort() leaves its input at S slots (:711): N
    // and S select the same op sequence (rotation amounts < N), so they share
    // a graph.
    GraphKey graphKey(const Ciphertext<DCRTPoly>& first, const std::vector<Ciphertext<DCRTPoly>>& cols,
                      SignFunc SignFunc, const SignConfig& Cfg, bool stable) {
        const sfhe::RankLayout L(N, max_batch);
        auto slotsOf = [&](const Ciphertext<DCRTPoly>& c) {
            return c->GetSlots() == (uint32_t)L.S ? (uint32_t)N : c->GetSlots();
        };
        GraphKey key;
        key.level = first->GetLevel();
        key.slots = slotsOf(first);
        key.func = (int)SignFunc;
        key.n = Cfg.compos.n;
        key.dg = Cfg.compos.dg;
        key.df = Cfg.compos.df;
        key.multDepth = Cfg.multDepth;
        key.stable = stable;
        for (const auto& c : cols) key.cols.emplace_back(c->GetLevel(), slotsOf(c));
        return key;
    }
    struct Graph {
        std::shared_ptr<CryptoContextImpl<DCRTPoly>::CapturedGraph> g;
        std::vector<Ciphertext<DCRTPoly>> in, out;  // sorter-owned buffers (records: keys first)
        GraphKey key;
    };
    // One cache per mode: a sorter may alternate plain, stable and record
    // sorts, and each replays its own graph.
    struct GraphCache {
        std::unique_ptr<Graph> graph;
        GraphKey warmKey;
        bool warm = false;
    };
    GraphCache m_plain, m_stable, m_records;
    bool m_graphOff = false;
    bool m_lastStable = false;  // the mode of the last sort (graphNodes reports its graph)

    static bool graphsEnabled() {
        const char* v = std::getenv("SFHE_GRAPH");
        return !v || *v != '0';
    }

    // body() run inside a capture region, every output settled there: the
    // graph must write their final rows (EndCapture settles the one it keeps).
    // Null when the backend refuses or abandons the capture: nothing ran, and
    // the sorter runs eagerly from then on, as after a body that throws.
    template <class F>
    std::shared_ptr<CryptoContextImpl<DCRTPoly>::CapturedGraph> captureRegion(F&& body,
                                                                             std::vector<Ciphertext<DCRTPoly>>& out) {
        if (m_cc->BeginCapture()) {
            try {
                out = body();
                for (auto& o : out) m_cc->Settle(o);
            } catch (...) {
                m_cc->EndCapture(nullptr);
                m_graphOff = true;
                throw;
            }
            if (auto g = m_cc->EndCapture(out.back())) return g;
        }
        m_graphOff = true;
        return nullptr;
    }

    // The graph protocol over one cache: the first call of a shape (key) runs
    // eager(in), which generates and encodes the masks; the second captures
    // eager over sorter-owned copies of the inputs; from then on a call copies
    // the caller's inputs into those buffers, launches the graph and clones
    // its outputs.  The callers' inputs get the slot counts eager leaves.
    template <class F>
    std::vector<Ciphertext<DCRTPoly>> runCached(GraphCache& cache, const GraphKey& key,
                                                const std::vector<Ciphertext<DCRTPoly>>& in, F&& eager) {
        std::unique_ptr<Graph>& graph = cache.graph;
        if (!(graph && graph->key == key)) {
            if (!(cache.warm && cache.warmKey == key)) {  // first call of this shape: eager, builds the masks
                cache.warm = true;
                cache.warmKey = key;
                return eager(in);
            }
            graph.reset();
            auto g = std::make_unique<Graph>();
            g->key = key;
            // sorter-owned input buffers (eager copies) in canonical form: a lazy
            // product's pending rows would be rescaled into a new buffer
            // INSIDE the graph, and replays would then ignore the copied-in input
            for (const auto& c : in) {
                m_cc->Settle(c);
                g->in.push_back(c->Clone());
                m_cc->Settle(g->in.back());
            }
            g->g = captureRegion([&] { return eager(g->in); }, g->out);
            if (!g->g) return eager(in);
            graph = std::move(g);
        } else {
            for (size_t c = 0; c < in.size(); ++c)
                if (graph->in[c] != in[c]) m_cc->CopyCiphertextInto(graph->in[c], in[c]);
        }
        m_cc->Launch(graph->g);
        std::vector<Ciphertext<DCRTPoly>> result;
        for (size_t c = 0; c < in.size(); ++c) in[c]->SetSlots(graph->in[c]->GetSlots());  // eager's side effect (:711)
        for (const auto& o : graph->out) {
            result.push_back(o->Clone());
            result.back()->SetSlots(o->GetSlots());
        }
        return result;
    }

  public:
    ~DirectSort() override {
        m_plain.graph.reset();
        m_stable.graph.reset();
        m_records.graph.reset();
        m_debugGraphs.reset();
    }
    // nodes of the captured sort of the last sort's mode (0: none yet / eager)
    size_t graphNodes() const {
        const auto& graph = (m_lastStable ? m_stable : m_plain).graph;
        if (graph) return m_cc->GraphNodes(graph->g);
        if (m_lastStable) return 0;
        return m_debugGraphs ? m_cc->GraphNodes(m_debugGraphs->rank) + m_cc->GraphNodes(m_debugGraphs->place) : 0;
    }
    // the captured sort's kernels of one family replayed alone (bench roofline)
    bool graphFamilyTime(uint32_t family, int reps, double* ms, uint64_t* launches, double* bytes) {
        const auto& graph = (m_lastStable ? m_stable : m_plain).graph;
        return graph && m_cc->GraphFamilyTime(graph->g, family, reps, ms, launches, bytes);
    }

    // Debug sorts (DebugEncryption: PRINT_PT decrypts of the input, the rank
    // and the output inside sort(), reference :755-770, as DirectSortTest
    // times them) replay TWO graphs -- the rank and the placement -- with the
    // three decrypts run eagerly between them, instead of running the whole
    // sort eagerly.
    struct DebugGraphs {
        std::shared_ptr<CryptoContextImpl<DCRTPoly>::CapturedGraph> rank, place;
        Ciphertext<DCRTPoly> in, rankOut, out;
        GraphKey key;
    };
    std::unique_ptr<DebugGraphs> m_debugGraphs;

    Ciphertext<DCRTPoly> sortDebug(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc, SignConfig& Cfg,
                                   const GraphKey& key) {
        if (!(m_debugGraphs && m_debugGraphs->key == key)) {
            if (!(m_plain.warm && m_plain.warmKey == key)) {  // first sort of this shape: eager, builds the masks
                m_plain.warm = true;
                m_plain.warmKey = key;
                return sortEager(input_array, SignFunc, Cfg);
            }
            m_debugGraphs.reset();
            auto g = std::make_unique<DebugGraphs>();
            g->key = key;
            m_cc->Settle(input_array);
            g->in = input_array->Clone();
            m_cc->Settle(g->in);
            std::cout << "\n===== Direct Sort Input Array: \n";
            PRINT_PT(m_enc, input_array);
            auto capture = [&](auto&& body, Ciphertext<DCRTPoly>& out) {
                std::vector<Ciphertext<DCRTPoly>> outs;
                auto cg = captureRegion([&] { return std::vector<Ciphertext<DCRTPoly>>{body()}; }, outs);
                if (cg) {
                    out = outs[0];
                    m_cc->Launch(cg);
                }
                return cg;
            };
            g->rank = capture([&] { return constructRank(g->in, SignFunc, Cfg); }, g->rankOut);
            if (!g->rank) {  // (a capture that failed ran nothing: the rest eagerly)
                auto ctx_Rank = constructRank(input_array, SignFunc, Cfg);
                std::cout << "\n===== Constructed Rank: \n";
                PRINT_PT(m_enc, ctx_Rank);
                auto output_array = rotationIndexCheckN(ctx_Rank, input_array);
                std::cout << "\n===== Final Output: \n";
                PRINT_PT(m_enc, output_array);
                std::cout << "Final Level: " << output_array->GetLevel() << std::endl;
                return output_array;
            }
            {
                const auto& ctx_Rank = g->rankOut;  // (PRINT_PT prints the expression's name)
                std::cout << "\n===== Constructed Rank: \n";
                PRINT_PT(m_enc, ctx_Rank);
            }
            g->place = capture([&] { return rotationIndexCheckN(g->rankOut, g->in); }, g->out);
            if (!g->place) {
                auto output_array = rotationIndexCheckN(g->rankOut, input_array);
                std::cout << "\n===== Final Output: \n";
                PRINT_PT(m_enc, output_array);
                std::cout << "Final Level: " << output_array->GetLevel() << std::endl;
                return output_array;
            }
            m_debugGraphs = std::move(g);
        } else {
            if (m_debugGraphs->in != input_array) m_cc->CopyCiphertextInto(m_debugGraphs->in, input_array);
            std::cout << "\n===== Direct Sort Input Array: \n";
            PRINT_PT(m_enc, input_array);
            m_cc->Launch(m_debugGraphs->rank);
            const auto& ctx_Rank = m_debugGraphs->rankOut;
            std::cout << "\n===== Constructed Rank: \n";
            PRINT_PT(m_enc, ctx_Rank);
            m_cc->Launch(m_debugGraphs->place);
        }
        DebugGraphs& g = *m_debugGraphs;
        const auto& output_array = g.out;
        std::cout << "\n===== Final Output: \n";
        PRINT_PT(m_enc, output_array);
        std::cout << "Final Level: " << output_array->GetLevel() << std::endl;
        input_array->SetSlots(g.in->GetSlots());  // sort()'s side effect on its input (:711)
        auto result = g.out->Clone();
        result->SetSlots(g.out->GetSlots());
        return result;
    }

    Ciphertext<DCRTPoly> sort(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                              SignConfig& Cfg) override {
        return sortMode(input_array, SignFunc, Cfg, false);
    }

    // sort() with the stable rank (constructRankStable): inputs with duplicate
    // values sort, equal values in input order.  One level more than sort():
    // the context needs sfhe::stableSortDepth levels from the input's level.
    Ciphertext<DCRTPoly> sortStable(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc, SignConfig& Cfg) {
        const int need = (int)input_array->GetLevel() + sfhe::stableSortDepth(N, Cfg.compos);
        if ((int)m_cc->GetMultiplicativeDepth() < need)
            throw OpenFHEException("stable sort: needs multiplicative depth " + std::to_string(need) +
                                   " (one level more than the plain sort for the tie term); the context has " +
                                   std::to_string(m_cc->GetMultiplicativeDepth()));
        return sortMode(input_array, SignFunc, Cfg, true);
    }

    Ciphertext<DCRTPoly> sortMode(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc, SignConfig& Cfg,
                                  bool stable) {
        const bool debug = dynamic_cast<const DebugEncryption*>(m_enc.get()) != nullptr;
        m_lastStable = stable;
        // (a stable debug sort runs eagerly: the two-graph debug replay is the plain sort's)
        if (m_graphOff || !graphsEnabled() || (debug && stable))
            return sortEager(input_array, SignFunc, Cfg, stable);
        const GraphKey key = graphKey(input_array, {}, SignFunc, Cfg, stable);
        if (debug) return sortDebug(input_array, SignFunc, Cfg, key);
        return runCached(stable ? m_stable : m_plain, key, {input_array},
                         [&](const std::vector<Ciphertext<DCRTPoly>>& in) {
                             return std::vector<Ciphertext<DCRTPoly>>{sortEager(in[0], SignFunc, Cfg, stable)};
                         })[0];
    }

    // ---- records: a key column and its payload columns sorted by the key ----
    // rank = the (stable) rank of the keys, then ONE placement of {keys,
    // cols...} (placeMany): first the sorted keys, then the sorted columns.
    // Payload values must lie in [-1, 1] like the keys: the placement's error
    // scales with |value|.  stable = true needs sfhe::stableSortDepth levels
    // (constructRankStable's check and message).  Graphs follow the sort's
    // protocol (runCached) with a cache of their own, over 1 + C sorter-owned
    // input buffers.
    size_t recordsGraphNodes() const { return m_records.graph ? m_cc->GraphNodes(m_records.graph->g) : 0; }

    std::vector<Ciphertext<DCRTPoly>> sortRecordsEager(const std::vector<Ciphertext<DCRTPoly>>& in,
                                                       SignFunc SignFunc, SignConfig& Cfg, bool stable) {
        auto ctx_Rank = stable ? constructRankStable(in[0], SignFunc, Cfg) : constructRank(in[0], SignFunc, Cfg);
        return placeMany(ctx_Rank, in);
    }

    // {sorted keys, sorted cols...}
    std::vector<Ciphertext<DCRTPoly>> sortRecords(const Ciphertext<DCRTPoly>& keys,
                                                  const std::vector<Ciphertext<DCRTPoly>>& cols, SignFunc SignFunc,
                                                  SignConfig& Cfg, bool stable) {
        std::vector<Ciphertext<DCRTPoly>> in{keys};
        in.insert(in.end(), cols.begin(), cols.end());
        if (stable) {
            const int need = (int)keys->GetLevel() + sfhe::stableSortDepth(N, Cfg.compos);
            if ((int)m_cc->GetMultiplicativeDepth() < need)
                throw OpenFHEException("stable record sort: needs multiplicative depth " + std::to_string(need) +
                                       " (one level more than the plain sort for the tie term); the context has " +
                                       std::to_string(m_cc->GetMultiplicativeDepth()));
        }
        const bool debug = dynamic_cast<const DebugEncryption*>(m_enc.get()) != nullptr;
        if (m_graphOff || !graphsEnabled() || debug) return sortRecordsEager(in, SignFunc, Cfg, stable);
        return runCached(m_records, graphKey(keys, cols, SignFunc, Cfg, stable), in,
                         [&](const std::vector<Ciphertext<DCRTPoly>>& cs) {
                             return sortRecordsEager(cs, SignFunc, Cfg, stable);
                         });
    }

    // (the stable sort's depth was checked by sortStable: lexRank, not constructRankStable)
    Ciphertext<DCRTPoly> sortEager(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                                   SignConfig& Cfg, bool stable = false) {
        std::cout << "\n===== Direct Sort Input Array: \n";
        PRINT_PT(m_enc, input_array);
        auto ctx_Rank = stable ? lexRank({input_array}, {false}, SignFunc, Cfg)
                               : constructRank(input_array, SignFunc, Cfg);
        std::cout << "\n===== Constructed Rank: \n";
        PRINT_PT(m_enc, ctx_Rank);
        auto output_array = rotationIndexCheckN(ctx_Rank, input_array);
        std::cout << "\n===== Final Output: \n";
        PRINT_PT(m_enc, output_array);
        std::cout << "Final Level: " << output_array->GetLevel() << std::endl;
        return output_array;
    }
};

// Compare-and-swap bitonic network over the N slots (reference
// src/sort_algo.h:1393-1487, same schedule: values / 255, stages k = 2..N,
// distances j = k/2..1, EvalBootstrap(ct, 2, 20) once the level passes 29,
// CompositeSign comparisons, * 255 at the end).  Per stage the reference
// masks the array four times and rotates each masked copy (four key
// switches); here the array is rotated by -j and +j ONCE, both rotations
// sharing one hoisted ModUp, and the masks are rotated in the clear instead
// (Rot(x (.) m, r) = Rot(x, r) (.) Rot(m, r)), so each stage's partner
// vectors are fused plaintext-weighted sums (EvalMultAddPlain) of three
// ciphertexts.  The swap c a + (1 - c) b is b + c (a - b): one
// ciphertext product instead of two.  Same levels as the reference.
template <int N>
class BitonicSort : public SortBase<N> {
  public:
    std::shared_ptr<Encryption> m_enc;

    BitonicSort(CryptoContext<DCRTPoly> cc, PublicKey<DCRTPoly> publicKey,
                std::vector<int> rotIndices, std::shared_ptr<Encryption> enc)
        : SortBase<N>(enc), m_enc(enc), m_cc(cc), m_PublicKey(publicKey), m_comp(enc),
          m_rot(cc, enc, rotIndices) {}

    Ciphertext<DCRTPoly> sort(const Ciphertext<DCRTPoly>& input_array, SignFunc SignFunc,
                              SignConfig& Cfg) override {
        auto cur = m_cc->EvalMult(input_array, 1.0 / 255);
        for (int k = 2; k <= N; k *= 2)
            for (int j = k / 2; j > 0; j /= 2) {
                std::cout << "Loop k: " << k << " j: " << j << "\n";
                if (cur->GetLevel() > kBootstrapLevel) cur = m_cc->EvalBootstrap(cur, 2, 20);
                cur = stage(cur, k, j, SignFunc, Cfg);
            }
        return m_cc->EvalMult(cur, 255.0);
    }

  private:
    static constexpr uint32_t kBootstrapLevel = 29;

    // slot i and its partner i ^ j (i < partner): `lo` marks the lower slot of
    // an ascending pair (bit k of i clear), `hi` the upper one; the
    // descending pairs likewise.  Rotated copies are what the hoisted
    // rotations of the array line up with.
    struct StageMasks {
        Plaintext ascLo, ascHi, desLo, desHi;          // at the slot
        Plaintext ascLoUp, desLoUp, ascHiDn, desHiDn;  // shifted by +j / -j
        Plaintext partnerUp, partnerDn;                // ascLoUp + desLoUp, ascHiDn + desHiDn
    };

    StageMasks& masks(int k, int j, uint32_t level) {
        auto key = std::make_tuple(k, j, level);
        auto it = m_masks.find(key);
        if (it != m_masks.end()) return it->second;
        std::vector<double> aL(N, 0), aH(N, 0), dL(N, 0), dH(N, 0);
        for (int i = 0; i < N; ++i) {
            const int l = i ^ j;
            if (i >= l) continue;
            ((i & k) ? dL : aL)[i] = 1;
            ((i & k) ? dH : aH)[l] = 1;
        }
        auto shift = [](const std::vector<double>& v, int by) {  // out[p] = v[p - by]
            std::vector<double> o(N);
            for (int p = 0; p < N; ++p) o[p] = v[((p - by) % N + N) % N];
            return o;
        };
        auto sum = [](std::vector<double> a, const std::vector<double>& b) {
            for (int p = 0; p < N; ++p) a[p] += b[p];
            return a;
        };
        auto pt = [&](const std::vector<double>& v) { return m_cc->MakeCKKSPackedPlaintext(v, 1, level); };
        StageMasks m;
        m.ascLo = pt(aL), m.ascHi = pt(aH), m.desLo = pt(dL), m.desHi = pt(dH);
        m.ascLoUp = pt(shift(aL, j)), m.desLoUp = pt(shift(dL, j));
        m.ascHiDn = pt(shift(aH, -j)), m.desHiDn = pt(shift(dH, -j));
        m.partnerUp = pt(sum(shift(aL, j), shift(dL, j)));
        m.partnerDn = pt(sum(shift(aH, -j), shift(dH, -j)));
        return m_masks.emplace(key, std::move(m)).first->second;
    }

    Ciphertext<DCRTPoly> stage(const Ciphertext<DCRTPoly>& x, int k, int j, SignFunc SignFunc, SignConfig& Cfg) {
        const StageMasks& m = masks(k, j, x->GetLevel());
        // up[p] = x[p - j] (lower slots moved onto their partners), dn[p] = x[p + j]
        auto r = m_rot.rotateMany(x, {-j, j});
        const auto& up = r[0];
        const auto& dn = r[1];
        // every slot's partner value
        auto partner = m_cc->EvalMultAddPlain({up, dn}, {m.partnerUp, m.partnerDn});
        // the pair's larger-if-ascending / smaller-if-ascending arrangements
        auto keep = m_cc->EvalMultAddPlain({up, x, dn, x}, {m.ascLoUp, m.ascLo, m.desHiDn, m.desHi});
        auto swap = m_cc->EvalMultAddPlain({up, x, dn, x}, {m.desLoUp, m.desLo, m.ascHiDn, m.ascHi});
        auto c = m_comp.compare(m_cc, partner, x, SignFunc, Cfg);
        return m_cc->EvalAdd(swap, m_cc->EvalMult(c, m_cc->EvalSub(keep, swap)));
    }

    CryptoContext<DCRTPoly> m_cc;
    PublicKey<DCRTPoly> m_PublicKey;
    Comparison m_comp;
    RotationComposer<N> m_rot;
    std::map<std::tuple<int, int, uint32_t>, StageMasks> m_masks;
};
