// lbcrypto-compatible C++ surface of the MI355X CKKS engine.
//
// The reference (oksuman/sorting-fhe) calls OpenFHE 1.1.4 through exactly
// this surface (SURVEY.md §8(b) lists every member used on the hot path);
// re-providing it lets the reference-shaped algorithm files in csrc/algo
// (sort_algo.h, sign.*, comparison.*, rotation.h, encryption.*) compile
// against the device engine unchanged.  Nothing here is OpenFHE code: the
// CKKS arithmetic below is this project's own RNS-CKKS over the primitive
// layer in csrc/prims.h (gfx950 kernels in the product build).
//
// Semantics kept from the reference's expectations:
//  * packed encoding with batch < n/2 replicates the vector periodically,
//    so SetSlots(k*N) is a pure metadata change;
//  * EvalRotate(ct, r>0) is a LEFT rotation (automorphism X -> X^(5^r));
//  * automatic rescaling: every multiplication (ct*ct, ct*pt, ct*double)
//    consumes exactly one level, additions none; operands at different
//    levels are aligned by a scale-exact level adjustment;
//  * EvalChebyshevSeriesPS consumes exactly OpenFHE's depth for the degree
//    (table in chebyshev.cpp), so per-N multDepth tables are consumed
//    exactly (DirectSortTest asserts final level == multDepth).
#pragma once

#include <algorithm>
#include <charconv>
#include <complex>
#include <cstddef>
#include <locale>
#include <fstream>
#include <cstdint>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "prims.h"

namespace lbcrypto {

using usint = uint32_t;

// ----------------------------------------------------------------------------
// Error type (OpenFHE throws OpenFHEException, a std::exception).
class OpenFHEException : public std::runtime_error {
  public:
    explicit OpenFHEException(const std::string& m) : std::runtime_error(m) {}
};
#define SFHE_THROW(msg) throw ::lbcrypto::OpenFHEException(std::string(__func__) + ": " + (msg))

struct DCRTPoly {};  // tag type: a device-resident RNS polynomial
class CryptoContextCKKSRNS {};

enum SecurityLevel { HEStd_128_classic, HEStd_192_classic, HEStd_256_classic, HEStd_NotSet };
enum PKESchemeFeature {
    PKE = 0x01,
    KEYSWITCH = 0x02,
    PRE = 0x04,
    LEVELEDSHE = 0x08,
    ADVANCEDSHE = 0x10,
    MULTIPARTY = 0x20,
    FHE = 0x40,
    SCHEMESWITCH = 0x80
};
enum ScalingTechnique { FIXEDMANUAL, FIXEDAUTO, FLEXIBLEAUTO, FLEXIBLEAUTOEXT, NORESCALE };
enum KeySwitchTechnique { BV, HYBRID };
// serialization formats (OpenFHE SerType::BINARY / JSON; see Serial below)
namespace SerType {
enum Kind { JSON = 0, BINARY = 1 };
}

template <class T>
class CCParams;

template <>
class CCParams<CryptoContextCKKSRNS> {
  public:
    void SetMultiplicativeDepth(uint32_t d) { multDepth = d; }
    uint32_t GetMultiplicativeDepth() const { return multDepth; }
    void SetScalingModSize(uint32_t b) { scalingModSize = b; }
    uint32_t GetScalingModSize() const { return scalingModSize; }
    void SetFirstModSize(uint32_t b) { firstModSize = b; }
    uint32_t GetFirstModSize() const { return firstModSize; }
    void SetBatchSize(uint32_t b) { batchSize = b; }
    uint32_t GetBatchSize() const { return batchSize; }
    void SetRingDim(uint32_t n) { ringDim = n; }
    uint32_t GetRingDim() const { return ringDim; }
    void SetSecurityLevel(SecurityLevel s) { securityLevel = s; }
    SecurityLevel GetSecurityLevel() const { return securityLevel; }
    void SetNumLargeDigits(uint32_t d) { numLargeDigits = d; }
    uint32_t GetNumLargeDigits() const { return numLargeDigits; }
    void SetScalingTechnique(ScalingTechnique t) { scalingTechnique = t; }
    ScalingTechnique GetScalingTechnique() const { return scalingTechnique; }
    void SetKeySwitchTechnique(KeySwitchTechnique t) { ksTech = t; }
    KeySwitchTechnique GetKeySwitchTechnique() const { return ksTech; }
    // Engine extensions (not in OpenFHE): device ordinal and RNG seed.
    void SetDevice(int d) { device = d; }
    int GetDevice() const { return device; }
    void SetSeed(uint64_t s) { seed = s; }
    uint64_t GetSeed() const { return seed; }

  private:
    uint32_t multDepth = 1;
    uint32_t scalingModSize = 50;
    uint32_t firstModSize = 60;
    uint32_t batchSize = 0;
    uint32_t ringDim = 0;
    SecurityLevel securityLevel = HEStd_128_classic;
    uint32_t numLargeDigits = 0;
    ScalingTechnique scalingTechnique = FLEXIBLEAUTOEXT;  // OpenFHE default
    KeySwitchTechnique ksTech = HYBRID;
    int device = 0;
    uint64_t seed = 0x5eed5eed2025ULL;
};

template <class E>
class CryptoContextImpl;
template <class E>
class CiphertextImpl;
template <class E>
class PublicKeyImpl;
template <class E>
class PrivateKeyImpl;
class PlaintextImpl;

template <class E>
using CryptoContext = std::shared_ptr<CryptoContextImpl<E>>;
template <class E>
using Ciphertext = std::shared_ptr<CiphertextImpl<E>>;
template <class E>
using ConstCiphertext = std::shared_ptr<const CiphertextImpl<E>>;
template <class E>
using PublicKey = std::shared_ptr<PublicKeyImpl<E>>;
template <class E>
using PrivateKey = std::shared_ptr<PrivateKeyImpl<E>>;
using Plaintext = std::shared_ptr<PlaintextImpl>;
using ConstPlaintext = std::shared_ptr<const PlaintextImpl>;

template <class E>
struct KeyPair {
    PublicKey<E> publicKey;
    PrivateKey<E> secretKey;
    bool good() const { return publicKey && secretKey; }
};

class DeviceBuffer;  // pooled device allocation (context.cpp)
using DeviceBufferPtr = std::shared_ptr<DeviceBuffer>;
struct DeferredOp;   // a product whose rescale awaits its consumer (context.cpp)

// ---------------------------------------------------------------------------
class EncodingParamsImpl {
  public:
    explicit EncodingParamsImpl(uint32_t b) : batch(b) {}
    uint32_t GetBatchSize() const { return batch; }

  private:
    uint32_t batch;
};
using EncodingParams = std::shared_ptr<EncodingParamsImpl>;

// ---------------------------------------------------------------------------
class PlaintextImpl {
  public:
    PlaintextImpl(std::vector<std::complex<double>> v, uint32_t slots, uint32_t level)
        : values(std::move(v)), slots(slots), level(level), length(slots) {}
    const std::vector<double>& GetRealPackedValue() const;
    const std::vector<std::complex<double>>& GetCKKSPackedValue() const { return values; }
    void SetLength(size_t len) { length = len; }
    size_t GetLength() const { return length; }
    uint32_t GetSlots() const { return slots; }
    uint32_t GetLevel() const { return level; }
    double GetLogPrecision() const { return logPrecision; }
    double GetLogError() const { return logError; }

    // engine internals
    std::vector<std::complex<double>> values;
    uint32_t slots;
    uint32_t level;
    size_t length;
    double logPrecision = 0.0;
    double logError = 0.0;
    mutable std::vector<double> realCache;
    std::map<uint32_t, DeviceBufferPtr> encoded;  // level -> device poly
    std::mutex encMutex;
};
std::ostream& operator<<(std::ostream& os, const Plaintext& pt);

// ---------------------------------------------------------------------------
template <>
class CiphertextImpl<DCRTPoly> {
  public:
    Ciphertext<DCRTPoly> Clone() const;
    uint32_t GetLevel() const { return level; }
    uint32_t GetSlots() const { return slots; }
    void SetSlots(uint32_t s) { slots = s; }
    double GetScalingFactor() const { return scale; }
    uint32_t GetNoiseScaleDeg() const { return 1; }
    CryptoContext<DCRTPoly> GetCryptoContext() const { return cc; }
    uint32_t GetNumLimbs() const;

    // engine internals: c0 / c1 are views into buf (limb-major rows).
    CryptoContext<DCRTPoly> cc;
    DeviceBufferPtr buf;
    uint64_t* c0 = nullptr;
    uint64_t* c1 = nullptr;
    uint32_t level = 0;
    uint32_t slots = 0;
    double scale = 1.0;
    // Lazy rescaling.  `level` is always the level AFTER the
    // product's rescale (what GetLevel reports and the level tables count).
    //  * def: the product is not computed yet (c0 / c1 unset); its first
    //    consumer picks the form it can use;
    //  * pend: the rows hold the product BEFORE its rescale (one limb more,
    //    scale = the product's scale): rotations and sums run on that form, so
    //    their key-switch and rescale rounding is divided away by the one
    //    rescale that settles the result.
    std::shared_ptr<DeferredOp> def;
    bool pend = false;
    // The form this ciphertext had before a graph capture computed or settled
    // it: the captured work only runs on replay, so if that
    // capture is abandoned the ciphertext returns to this form and is
    // recomputed eagerly by its next consumer.
    struct CaptureUndo {
        uint64_t epoch = 0;
        std::shared_ptr<DeferredOp> def;
        DeviceBufferPtr buf;
        uint64_t *c0 = nullptr, *c1 = nullptr;
        bool pend = false;
        double scale = 1.0;
    };
    std::shared_ptr<CaptureUndo> undo;
};

// Key pairs carry a random 64-bit tag (OpenFHE's keyTag): evaluation keys,
// ciphertexts and their serialized records name the key pair they belong to.
std::string KeyTagString(uint64_t tag);
template <>
class PublicKeyImpl<DCRTPoly> {
  public:
    DeviceBufferPtr b, a;  // over Q (L+1 limbs), evaluation domain
    CryptoContext<DCRTPoly> cc;
    uint64_t tag = 0;
    std::string GetKeyTag() const { return KeyTagString(tag); }
};
template <>
class PrivateKeyImpl<DCRTPoly> {
  public:
    DeviceBufferPtr s;            // over Q u P, evaluation domain
    std::vector<int8_t> ternary;  // coefficient form, for export / tests
    CryptoContext<DCRTPoly> cc;
    uint64_t tag = 0;
    std::string GetKeyTag() const { return KeyTagString(tag); }
};

// Hoisted-rotation digits (EvalFastRotationPrecompute result).
struct FastRotationPrecomp {
    DeviceBufferPtr ext;
    uint32_t level = 0;
    bool pend = false;  // taken of the ciphertext's unrescaled rows (one limb more)
    uint32_t beta = 0;
    size_t stride = 0;
    // pending precomputations pin the c0 rows they were taken with: another
    // consumer may settle (rescale) the shared ciphertext before the rotations
    DeviceBufferPtr pinBuf;
    const uint64_t* pinC0 = nullptr;
};

struct SfheContextState;  // parameters, tables, keys, pools (context.cpp)

// ---------------------------------------------------------------------------
template <>
class CryptoContextImpl<DCRTPoly> : public std::enable_shared_from_this<CryptoContextImpl<DCRTPoly>> {
  public:
    explicit CryptoContextImpl(const CCParams<CryptoContextCKKSRNS>& p);
    ~CryptoContextImpl();

    void Enable(PKESchemeFeature f) { enabled |= f; }
    void Enable(uint32_t mask) { enabled |= mask; }

    uint32_t GetRingDimension() const;
    uint32_t GetCyclotomicOrder() const { return 2 * GetRingDimension(); }
    EncodingParams GetEncodingParams() const;
    uint32_t GetMultiplicativeDepth() const;

    // keys
    KeyPair<DCRTPoly> KeyGen();
    void EvalMultKeyGen(const PrivateKey<DCRTPoly>& sk);
    void EvalRotateKeyGen(const PrivateKey<DCRTPoly>& sk, const std::vector<int32_t>& idx,
                          const PublicKey<DCRTPoly>& pk = nullptr);
    void EvalAtIndexKeyGen(const PrivateKey<DCRTPoly>& sk, const std::vector<int32_t>& idx) {
        EvalRotateKeyGen(sk, idx);
    }
    void ClearEvalMultKeys();
    void ClearEvalAutomorphismKeys();
    // Key serialization (OpenFHE's static forms).  Each record names its
    // context's parameter fingerprint and its key pair's tag; keyTag = ""
    // writes the evaluation keys of every registered context, a tag only
    // those of the key pair with that tag.  Deserialization installs a
    // record into a context with the record's fingerprint that holds no key
    // pair yet (the newest one: a context deserialized before its keys), or
    // else into the context that holds the record's own key pair -- never
    // into a context of another key pair.
    static bool SerializeEvalMultKey(std::ostream& os, SerType::Kind k, const std::string& keyTag = "");
    static bool DeserializeEvalMultKey(std::istream& is, SerType::Kind k);
    static bool SerializeEvalAutomorphismKey(std::ostream& os, SerType::Kind k, const std::string& keyTag = "");
    static bool DeserializeEvalAutomorphismKey(std::istream& is, SerType::Kind k);
    // parameter fingerprint: ring, prime chain, special primes, digits, scales
    uint64_t Fingerprint() const;
    // tag of the key pair this context's evaluation keys belong to (0: none yet)
    uint64_t KeyTag() const;
    const CCParams<CryptoContextCKKSRNS>& GetParams() const;
    uint32_t GetEnabledMask() const { return enabled; }

    // encode / encrypt / decrypt
    Plaintext MakeCKKSPackedPlaintext(const std::vector<double>& v, uint32_t scaleDeg = 1,
                                      uint32_t level = 0, const void* params = nullptr,
                                      uint32_t slots = 0) const;
    Plaintext MakeCKKSPackedPlaintext(const std::vector<std::complex<double>>& v,
                                      uint32_t scaleDeg = 1, uint32_t level = 0,
                                      const void* params = nullptr, uint32_t slots = 0) const;
    Ciphertext<DCRTPoly> Encrypt(const PublicKey<DCRTPoly>& pk, const Plaintext& pt);
    Ciphertext<DCRTPoly> Encrypt(const Plaintext& pt, const PublicKey<DCRTPoly>& pk) {
        return Encrypt(pk, pt);
    }
    // Engine extension: the encryptions of pts (any mix of levels and slot
    // counts), residue for residue what Encrypt gives on each in list order (the
    // sampling seeds are drawn in that order).  Where the backend samples on the
    // device (prims.h sfp_sample_small, sfp_encrypt_combine) a level's
    // plaintexts cost one sampling launch, one batched NTT and one combining
    // launch, with no device drain; elsewhere it is a loop over Encrypt.
    std::vector<Ciphertext<DCRTPoly>> EncryptMany(const PublicKey<DCRTPoly>& pk, const std::vector<Plaintext>& pts);
    void Decrypt(const PrivateKey<DCRTPoly>& sk, const Ciphertext<DCRTPoly>& ct, Plaintext* out);
    void Decrypt(const Ciphertext<DCRTPoly>& ct, const PrivateKey<DCRTPoly>& sk, Plaintext* out) {
        Decrypt(sk, ct, out);
    }
    // Engine extension: outs[k] = the decryption of cts[k] (any mix of levels
    // and slot counts), the same plaintexts as Decrypt on each.  Where the
    // backend decodes on the device (prims.h sfp_decode_batch) the batch costs
    // one inverse NTT and one decode per (slots, limbs) group, one download and
    // one synchronisation; elsewhere it is a loop over Decrypt.
    void DecryptMany(const PrivateKey<DCRTPoly>& sk, const std::vector<Ciphertext<DCRTPoly>>& cts,
                     std::vector<Plaintext>* outs);

    // additive
    Ciphertext<DCRTPoly> EvalAdd(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b);
    Ciphertext<DCRTPoly> EvalAdd(const Ciphertext<DCRTPoly>& a, double c);
    Ciphertext<DCRTPoly> EvalAdd(double c, const Ciphertext<DCRTPoly>& a) { return EvalAdd(a, c); }
    Ciphertext<DCRTPoly> EvalAdd(const Ciphertext<DCRTPoly>& a, const Plaintext& p);
    Ciphertext<DCRTPoly> EvalAdd(const Plaintext& p, const Ciphertext<DCRTPoly>& a) {
        return EvalAdd(a, p);
    }
    void EvalAddInPlace(Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b);
    void EvalAddInPlace(Ciphertext<DCRTPoly>& a, double c);
    void EvalAddInPlace(Ciphertext<DCRTPoly>& a, const Plaintext& p);
    Ciphertext<DCRTPoly> EvalSub(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b);
    Ciphertext<DCRTPoly> EvalSub(const Ciphertext<DCRTPoly>& a, double c) { return EvalAdd(a, -c); }
    Ciphertext<DCRTPoly> EvalSub(double c, const Ciphertext<DCRTPoly>& a);
    Ciphertext<DCRTPoly> EvalSub(const Ciphertext<DCRTPoly>& a, const Plaintext& p);
    Ciphertext<DCRTPoly> EvalSub(const Plaintext& p, const Ciphertext<DCRTPoly>& a);
    void EvalSubInPlace(Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b);
    void EvalSubInPlace(Ciphertext<DCRTPoly>& a, double c) { EvalAddInPlace(a, -c); }
    Ciphertext<DCRTPoly> EvalNegate(const Ciphertext<DCRTPoly>& a);
    void EvalNegateInPlace(Ciphertext<DCRTPoly>& a);
    Ciphertext<DCRTPoly> EvalAddMany(const std::vector<Ciphertext<DCRTPoly>>& v);

    // multiplicative (automatic rescale: +1 level each)
    Ciphertext<DCRTPoly> EvalMult(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b);
    Ciphertext<DCRTPoly> EvalMult(const Ciphertext<DCRTPoly>& a, double c);
    Ciphertext<DCRTPoly> EvalMult(double c, const Ciphertext<DCRTPoly>& a) { return EvalMult(a, c); }
    Ciphertext<DCRTPoly> EvalMult(const Ciphertext<DCRTPoly>& a, const Plaintext& p);
    Ciphertext<DCRTPoly> EvalMult(const Plaintext& p, const Ciphertext<DCRTPoly>& a) {
        return EvalMult(a, p);
    }
    void EvalMultInPlace(Ciphertext<DCRTPoly>& a, double c);
    void EvalMultInPlace(Ciphertext<DCRTPoly>& a, const Plaintext& p);
    Ciphertext<DCRTPoly> EvalMultAndRelinearize(const Ciphertext<DCRTPoly>& a,
                                                const Ciphertext<DCRTPoly>& b) {
        return EvalMult(a, b);
    }
    Ciphertext<DCRTPoly> EvalSquare(const Ciphertext<DCRTPoly>& a);
    // Engine extension (the stable rank sort's tie-aware term):
    // s (.) (W (.) s + k), relinearised, at s's level + 2 -- the value of
    // EvalMult(s, EvalAdd(EvalMult(s, W), k)) with the product kept lazy over
    // its three factors (two rescales at the end, the relinearisation before
    // both).  The tensor is one launch where the backend has prims.h
    // sfp_tie_tensor; elsewhere (the C oracle, SFHE_TIE_FUSED=0 -- read per
    // call --, a level whose rows are dealt over ranks, or the prim declining)
    // sfp_mul, sfp_add_const and sfp_tensor compose the same integers.
    // OpStats tie_fused / tie_composed count the calls of each kind.
    Ciphertext<DCRTPoly> EvalTieTerm(const Ciphertext<DCRTPoly>& s, const Plaintext& W, double k);
    // Engine extension (the lexicographic rank's Horner step):
    // v + (1 - q) (.) u, relinearised, one level below u, from a single
    // relinearisation and a single rescale.  q and v may have more limbs than
    // u (a numerically lower level) and are read over u's limbs.  q keeps its
    // own scale Delta_q: the constant 1 enters as the residues of Delta_q and v
    // is lifted by the integer round(Delta_q Delta_u / Delta_v), so the three
    // summands of the tensor carry one scale and their sum is exact.  The
    // result's scale field holds Delta_q Delta_u / q_dropped (the level's
    // nominal scale up to the drift between two levels' scales, ~1e-7
    // relative); the next step, level adjustments and decryption read that
    // field.  The tensor is one launch where the backend has prims.h
    // sfp_lex_tensor; elsewhere (the C oracle, SFHE_LEX_FUSED=0 -- read per
    // call --, a level whose rows are dealt over ranks, or the prim declining)
    // the generic prims compose the same integers.  OpStats lex_fused /
    // lex_composed count the calls of each kind.
    Ciphertext<DCRTPoly> EvalLexStep(const Ciphertext<DCRTPoly>& v, const Ciphertext<DCRTPoly>& q,
                                     const Ciphertext<DCRTPoly>& u);
    // Engine extension (the grouping's gated column sums):
    // out[c] = sum_b (1 - q[b]) (.) u[c][b], relinearised ONCE per column, one
    // level below q.  The B gates q[b] share one level and one scale and serve
    // all C <= kGateMaxColumns columns; column c's operands u[c][b] share one
    // scale and have at least q's limbs (a numerically lower or equal level):
    // they are read over q's limbs.  The constant 1 enters as the residues of
    // Delta_q, so every product carries Delta_q Delta_u and the sum is exact;
    // the result's scale field holds Delta_q Delta_u / q_dropped (EvalLexStep).
    // The tensors of all batches and columns are one launch per tile of two
    // columns where the backend has prims.h sfp_gate_tensor_cols and B <=
    // SFP_GATE_MAX_B; elsewhere (the C oracle, SFHE_GROUP_FUSED=0 -- read per
    // call --, a level whose rows are dealt over ranks, more batches, or the
    // prim declining) the generic prims compose the same integers.  OpStats
    // gate_fused / gate_composed count the calls of each kind.
    static constexpr size_t kGateMaxColumns = 8;
    std::vector<Ciphertext<DCRTPoly>> EvalGateSumMany(const std::vector<Ciphertext<DCRTPoly>>& q,
                                                      const std::vector<std::vector<Ciphertext<DCRTPoly>>>& u);
    // Engine extension (the window sums' weighted column sums):
    // out[c] = sum_b (p[b] + v[b]) (.) u[c][b], relinearised ONCE per column,
    // one level below v.  The B gates are a ciphertext v[b] plus a per-slot
    // plaintext p[b]: the v[b] share one level and one scale, every p[b] is a
    // plaintext over at least v's limbs and is encoded at v's scale field, so
    // p + v is exact.  The gates serve all C <= kGateMaxColumns columns;
    // column c's operands u[c][b] share one scale and have at least v's limbs
    // (a numerically lower or equal level): they are read over v's limbs.
    // The result's scale field holds Delta_v Delta_u / q_dropped
    // (EvalLexStep).  The tensors of all batches and columns are one launch
    // per tile of two columns where the backend has prims.h
    // sfp_weight_tensor_cols and B <= SFP_WEIGHT_MAX_B; elsewhere (the C
    // oracle, SFHE_WINDOW_FUSED=0 -- read per call --, a level whose rows are
    // dealt over ranks, more batches, or the prim declining) the generic prims
    // compose the same integers.  OpStats weight_fused / weight_composed count
    // the calls of each kind.
    std::vector<Ciphertext<DCRTPoly>> EvalWeightSumMany(const std::vector<Ciphertext<DCRTPoly>>& v,
                                                        const std::vector<Plaintext>& p,
                                                        const std::vector<std::vector<Ciphertext<DCRTPoly>>>& u);
    // Engine extension (the OR of two gates: a join on several keys, DESIGN.md
    // §4l): a + b - a (.) b, relinearised, one level below the lower operand,
    // from a single relinearisation and a single rescale.  a and b keep their
    // own scales Delta_a, Delta_b and may sit at different levels: the one
    // with more limbs is read over the other's limbs (EvalGateSumMany's rule).
    // The linear terms enter as kb a + ka b with ka, kb the residues of
    // Delta_a, Delta_b (formed as EvalLexStep's kr), so the three summands of
    // the tensor carry Delta_a Delta_b and their sum is exact; the result's
    // scale field holds Delta_a Delta_b / q_dropped.  The tensor is one launch
    // where the backend has prims.h sfp_or_tensor; elsewhere (the C oracle,
    // SFHE_JOIN_FUSED=0 -- read per call --, a level whose rows are dealt over
    // ranks, or the prim declining) the generic prims compose the same
    // integers.  OpStats or_fused / or_composed count the calls of each kind.
    Ciphertext<DCRTPoly> EvalGateOr(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b);
    // Engine extension: EvalMult(a_i, b_i) for independent pairs, each formed
    // canonically (rescaled: the values a lazy product takes when its
    // consumer needs the canonical form); pairs at one level run as batched
    // ops (prims.h sfp_batch_*: their identical launches merged, up to four
    // pairs per launch).
    std::vector<Ciphertext<DCRTPoly>> EvalMultMany(const std::vector<Ciphertext<DCRTPoly>>& a,
                                                   const std::vector<Ciphertext<DCRTPoly>>& b);
    // Engine extension (the polynomial evaluators): EvalMult(a, b) followed by
    // EvalAdd / EvalSub of a ciphertext r (sign < 0: subtract) and / or
    // EvalAdd of a constant c -- the same values.  Where the product takes
    // the fused canonical path at an unsharded level, no operand is lazy, and
    // r is settled at exactly the product's level with that level's scale
    // and the output's layout, the sum rides in the last pass of the
    // product's rescale (prims.h sfp_*_add) instead of a launch of its own;
    // everywhere else the separate ops run.  SFHE_PS_FMA=0: always separate.
    struct MultAddend {
        Ciphertext<DCRTPoly> r;
        int sign = 1;
        double c = 0.0;
    };
    Ciphertext<DCRTPoly> EvalMultAdd(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b,
                                     const MultAddend& add);
    // ... for independent pairs, batched as EvalMultMany's
    std::vector<Ciphertext<DCRTPoly>> EvalMultManyAdd(const std::vector<Ciphertext<DCRTPoly>>& a,
                                                      const std::vector<Ciphertext<DCRTPoly>>& b,
                                                      const std::vector<MultAddend>& adds);
    // Engine extension (the sign polynomials' paired products):
    // Rescale(Relin(a (x) b + a2 (x) b2)) + r, one level below the operands --
    // the value of EvalAdd(EvalAdd(EvalMult(a, b), EvalMult(a2, b2)), r) with
    // the two tensors summed before ONE relinearisation, ModDown and rescale
    // (one key-switch rounding instead of two).  Throws unless the four
    // operands are settled (no deferred or pending product: Settle), at one
    // level, with a.scale * b.scale == a2.scale * b2.scale, and r (may be null)
    // is settled at the result's level with that level's scale.  The composed
    // form defines the integers: sfp_tensor twice, the three components summed
    // (sfp_add), the relinearisation with its fused ModDown + rescale, the sum
    // with r.  Where the backend has prims.h sfp_mult2_relin_rescale_add it is
    // one product's launch chain that reads the second pair where it reads the
    // first; elsewhere (the C oracle, SFHE_MULT_SUM2_FUSED=0 -- read per call --,
    // SFHE_FUSED_RESCALE=0, a level whose rows are dealt over ranks, the prim
    // declining) the composed form runs: the same residues.  OpStats dot_fused
    // / dot_composed count the calls of each kind.
    Ciphertext<DCRTPoly> EvalMultSum2(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b,
                                      const Ciphertext<DCRTPoly>& a2, const Ciphertext<DCRTPoly>& b2,
                                      const Ciphertext<DCRTPoly>& r);
    // Engine extension (the Chebyshev evaluator's remainder chains, DESIGN.md
    // §4b): Rescale(Relin(sum_i a_i (x) b_i)) + addend for 1 <= m <=
    // kMultSumMaxTerms terms, one level below the operands -- EvalMultSum2's
    // contract with m pairs: every operand settled, all 2m at one level,
    // a_i.scale * b_i.scale equal for all i; the addend's r null or canonical
    // at the result's level (added, or subtracted with sign < 0), its constant
    // c added at the result's scale.  A violation throws.  The composed form
    // defines the integers: m sfp_tensor, their components summed (sfp_add),
    // one relinearisation with its fused ModDown + rescale, then the addend.
    // m = 2 gives EvalMultSum2's residues, m = 1 EvalMultAdd's.  Where the
    // backend has prims.h sfp_multn_relin_rescale_add the sum is one
    // product's launch chain; elsewhere (the C oracle, SFHE_MULT_SUM_FUSED=0
    // -- read per call --, SFHE_FUSED_RESCALE=0, a level whose rows are dealt
    // over ranks, the prim declining) the composed form runs: the same
    // residues.  OpStats sumn_fused / sumn_composed count the ops of each kind.
    static constexpr uint32_t kMultSumMaxTerms = 8;
    using MultTerm = std::pair<Ciphertext<DCRTPoly>, Ciphertext<DCRTPoly>>;
    struct MultSumOp {
        std::vector<MultTerm> terms;
        MultAddend add;
    };
    Ciphertext<DCRTPoly> EvalMultSum(const std::vector<MultTerm>& terms, const MultAddend& add);
    // ... for independent ops: consecutive ops of one level AND one term count
    // go out as one batch (EvalMultMany's path, runs of up to BatchWidth());
    // ops of different term counts never share a batch
    std::vector<Ciphertext<DCRTPoly>> EvalMultSumMany(const std::vector<MultSumOp>& ops);
    // the condition of EvalMultSum that op violates (a message), or null
    const char* MultSumViolation(const MultSumOp& op) const;
    // Engine extension: sum_i a_i * p_i with ONE rescale (same value and
    // level as summing the individually rescaled EvalMult(a_i, p_i)).
    Ciphertext<DCRTPoly> EvalMultAddPlain(const std::vector<Ciphertext<DCRTPoly>>& a,
                                          const std::vector<Plaintext>& p);
    // Engine extension (records: several columns placed by one rank, DESIGN.md
    // §4f): out[c][g] = EvalMultAddPlain(a[c], *p[g]) for columns a[c] of one
    // length under the SAME plaintext sets.  Where the backend has prims.h
    // sfp_mac_plain2_cols the sums are formed at once, pending (unrescaled, as
    // EvalRotateSum takes them), by launches that read each plaintext once for
    // a tile of columns; elsewhere (the C oracle, SFHE_PLACE_COLS=0 -- read per
    // call --, operands of different levels, the prim declining) they stay
    // deferred and each column takes today's path.  The same residues.
    // OpStats place_fused / place_composed count the sums of each kind.
    std::vector<std::vector<Ciphertext<DCRTPoly>>> EvalMultAddPlainCols(
        const std::vector<std::vector<Ciphertext<DCRTPoly>>>& a, const std::vector<const std::vector<Plaintext>*>& p);
    // a multi-column placement evaluated `hits` indicators for `columns` columns (OpStats)
    void NotePlacement(uint64_t hits, uint64_t columns);

    // rotations
    Ciphertext<DCRTPoly> EvalRotate(const Ciphertext<DCRTPoly>& a, int32_t r);
    Ciphertext<DCRTPoly> EvalAtIndex(const Ciphertext<DCRTPoly>& a, int32_t r) {
        return EvalRotate(a, r);
    }
    std::shared_ptr<FastRotationPrecomp> EvalFastRotationPrecompute(const Ciphertext<DCRTPoly>& a);
    Ciphertext<DCRTPoly> EvalFastRotation(const Ciphertext<DCRTPoly>& a, int32_t r, uint32_t m,
                                          const std::shared_ptr<FastRotationPrecomp>& pre);
    // Engine extension: sum_k EvalRotate(a_k, r_k) with the key switches'
    // inner products summed in the extended basis Q*P and ONE ModDown (output
    // aggregation).  The same value as EvalAddMany of the rotations, with one
    // ModDown rounding instead of one per term.  Every r_k needs its own key.
    Ciphertext<DCRTPoly> EvalRotateSum(const std::vector<Ciphertext<DCRTPoly>>& a,
                                       const std::vector<int32_t>& r);
    // Engine extension (the selection's in-partition sums):
    // sum_{k < count} EvalRotate(a, k * stride), 2 <= count <= 8, with ONE
    // ModUp (the rotations of one ciphertext share its extended digits, as
    // EvalFastRotation), the key inner products of all rotating terms summed in
    // the extended basis and ONE ModDown (as EvalRotateSum).  Term 0 is `a`
    // itself, and a term whose amount is a multiple of the slot count is added
    // as it is; every other amount needs its own rotation key (the error names
    // the amount).  Where the backend has prims.h sfp_ks_inner_aut_sum the
    // inner products are one launch that reads the digits through every
    // automorphism; elsewhere (the C oracle, SFHE_SELECT_FOLD=0 -- read per
    // call --, a level whose rows are dealt over ranks, the prim declining) each
    // term permutes the digits (sfp_automorph) and accumulates
    // (sfp_ks_inner / sfp_ks_inner_acc): the same residues.  OpStats
    // fold_fused / fold_composed count the calls of each kind.
    Ciphertext<DCRTPoly> EvalRotateFold(const Ciphertext<DCRTPoly>& a, int32_t stride, uint32_t count);
    // Engine extension (a selection's payload columns): the
    // results of EvalRotateFold(a[c], stride, count), residue for residue, for
    // a non-empty list of ciphertexts at one level and slot count.  The terms,
    // keys and tier check are derived once; each column keeps its ModUp, its
    // sum of sigma_k(c0) and its ModDown; the columns' inner products are one
    // prims.h sfp_ks_inner_aut_sum_cols call (tiles of columns that read each
    // key word once).  Elsewhere (the C oracle, SFHE_SELECT_COLS=0 -- read per
    // call --, a level whose rows are dealt over ranks, no rotating term, the
    // prim declining) it is EvalRotateFold per column.  OpStats
    // fold_cols_fused counts the prim's launches, fold_cols_composed the
    // columns that went through EvalRotateFold.
    std::vector<Ciphertext<DCRTPoly>> EvalRotateFoldMany(const std::vector<Ciphertext<DCRTPoly>>& a, int32_t stride,
                                                         uint32_t count);
    // a selection ran `batches` indicator batches (OpStats)
    void NoteSelection(uint64_t batches);
    // ... and served `columns` columns with them
    void NoteSelectionColumns(uint64_t columns);
    // Engine extension (double hoisting): sum_t sum_k p_tk (.) EvalRotate(a_t, r_tk), then one
    // rescale -- EvalMultAddPlain over hoisted rotations.  Each input's rotations share one
    // ModUp; every key-switched term is multiplied by its plaintext in the extended basis Q*P
    // and the whole sum takes ONE ModDown (one per rotation otherwise).
    Ciphertext<DCRTPoly> EvalRotMultAddHoisted(
        const std::vector<Ciphertext<DCRTPoly>>& a,
        const std::vector<std::vector<std::pair<int32_t, Plaintext>>>& terms);

    // polynomial evaluation (chebyshev.cpp)
    Ciphertext<DCRTPoly> EvalChebyshevSeriesPS(const Ciphertext<DCRTPoly>& x,
                                               const std::vector<double>& coeffs, double a,
                                               double b);
    Ciphertext<DCRTPoly> EvalChebyshevSeries(const Ciphertext<DCRTPoly>& x,
                                             const std::vector<double>& coeffs, double a,
                                             double b) {
        return EvalChebyshevSeriesPS(x, coeffs, a, b);
    }
    Ciphertext<DCRTPoly> EvalChebyshevFunction(std::function<double(double)> f,
                                               const Ciphertext<DCRTPoly>& x, double a, double b,
                                               uint32_t degree);
    Ciphertext<DCRTPoly> EvalPolyLinear(const Ciphertext<DCRTPoly>& x,
                                        const std::vector<double>& coeffs);
    Ciphertext<DCRTPoly> EvalPoly(const Ciphertext<DCRTPoly>& x,
                                  const std::vector<double>& coeffs) {
        return EvalPolyLinear(x, coeffs);
    }

    // level management
    Ciphertext<DCRTPoly> Rescale(const Ciphertext<DCRTPoly>& a);
    Ciphertext<DCRTPoly> ModReduce(const Ciphertext<DCRTPoly>& a) { return Rescale(a); }
    void LevelReduceInPlace(Ciphertext<DCRTPoly>& a, std::nullptr_t, size_t levels);
    Ciphertext<DCRTPoly> AdjustLevel(const Ciphertext<DCRTPoly>& a, uint32_t targetLevel);
    // Engine internals of CKKS bootstrapping (bootstrap.cpp):
    //  * AdjustLevelScaled: AdjustLevel that also multiplies the values by
    //    `factor` (folded into the level adjustment's constant; no extra level);
    //  * ModRaise: a ciphertext at the last level (one limb, q_0) lifted to the
    //    whole chain: its centred residues mod q_0 taken as integers, so it now
    //    decrypts to m + q_0 I(X) at level 0 (labelled with level 0's scale);
    //  * EvalConjugate: slot-wise complex conjugation (automorphism X -> X^-1)
    //    with the key EvalConjugateKeyGen makes.
    Ciphertext<DCRTPoly> AdjustLevelScaled(const Ciphertext<DCRTPoly>& a, uint32_t targetLevel, double factor);
    Ciphertext<DCRTPoly> ModRaise(const Ciphertext<DCRTPoly>& a);
    Ciphertext<DCRTPoly> EvalConjugate(const Ciphertext<DCRTPoly>& a);
    void EvalConjugateKeyGen(const PrivateKey<DCRTPoly>& sk);

    // bootstrapping (needed only by the k-way / bitonic rows; link-only here)
    void EvalBootstrapSetup(std::vector<uint32_t> levelBudget, std::vector<uint32_t> dim1 = {0, 0},
                            uint32_t slots = 0, uint32_t correctionFactor = 0);
    void EvalBootstrapKeyGen(const PrivateKey<DCRTPoly>& sk, uint32_t slots);
    Ciphertext<DCRTPoly> EvalBootstrap(const Ciphertext<DCRTPoly>& ct, uint32_t numIterations = 1,
                                       uint32_t precision = 0);
    // Engine extensions: the levels EvalBootstrap consumes (counted from the
    // top of the chain: its output level), and one bootstrapping pass with
    // the values scaled by inFactor on the way in and outFactor on the way out
    uint32_t GetBootstrapDepth(const std::vector<uint32_t>& levelBudget, uint32_t slots = 0) const;
    Ciphertext<DCRTPoly> BootstrapOnce(const Ciphertext<DCRTPoly>& ct, double inFactor, double outFactor);
    // EvalBootstrap's passes (meta-bootstrapping for numIterations >= 2)
    Ciphertext<DCRTPoly> bootstrapIters(const Ciphertext<DCRTPoly>& ct, uint32_t numIterations, uint32_t precision);
    // ... replayed from a hipGraph captured per (input level, iterations,
    // precision) after the first eager call of that shape (bootstrap.cpp)
    Ciphertext<DCRTPoly> bootstrapReplay(const Ciphertext<DCRTPoly>& ct, uint32_t numIterations, uint32_t precision);
    // bootstrap shapes replayed from a captured graph so far
    size_t BootstrapGraphs() const;
    // Diagnostics (tools/prec_probe boot; not for production): called after
    // every bootstrapping stage of BootstrapOnce with the stage's output and,
    // for the linear stages (CoeffsToSlots / SlotsToCoeffs groups), the slot
    // map applied: out[p] = sum_k v_k[p] in[(p + k) mod S] (the first
    // SlotsToCoeffs group takes in = re + i im).  Stages: "low", "raised",
    // "traced", "c2s", "yre", "yim", "wre", "wim", "s2c".  Bootstraps run
    // eagerly while a tap is set.
    using BootstrapSlotMap = std::map<uint32_t, std::vector<std::complex<double>>>;
    using BootstrapTap =
        std::function<void(const char* stage, const Ciphertext<DCRTPoly>& ct, const BootstrapSlotMap* map)>;
    void SetBootstrapTap(BootstrapTap tap) { bootTap = std::move(tap); }
    // K + 1 of EvalMod's input scaling (y = x / (K + 1)) and the number of
    // double angles (diagnostics)
    static double BootstrapOverflowBound();
    static uint32_t BootstrapDoubleAngles();
    static uint32_t BootstrapChebDegree();

    // ---------------- engine extensions (not OpenFHE) ----------------
    SfheContextState* state() const { return st.get(); }
    // Galois element for a left rotation by r.
    uint32_t GaloisForRotation(int32_t r) const;
    bool HasRotationKey(int32_t r) const;
    // sum_j w_j * ct_j followed by one rescale to level + 1: the Chebyshev-
    // leaf kernel.  ct_j is given as c0/c1 device rows; its first ellOf(level)
    // rows are used, so an input at a LOWER level (more limbs) enters without
    // a level adjustment: inScale[j] (its scale; nullptr: every input at
    // Delta_level) is folded into its integer weight, which removes the
    // adjustment's rescale and its rounding noise.
    Ciphertext<DCRTPoly> LinearWSumRescale(const std::vector<const uint64_t*>& in0,
                                           const std::vector<const uint64_t*>& in1,
                                           const std::vector<double>& w, uint32_t level,
                                           uint32_t slots, const std::vector<double>* inScale = nullptr);
    // ... + constant (EvalAdd(out, constant)'s value: in the rescale's last
    // pass where the backend has that form)
    Ciphertext<DCRTPoly> LinearWSumRescale(const std::vector<const uint64_t*>& in0,
                                           const std::vector<const uint64_t*>& in1,
                                           const std::vector<double>& w, uint32_t level,
                                           uint32_t slots, const std::vector<double>* inScale, double constant);
    // A call with one input at a level whose rows are not dealt over ranks is
    // a constant rescale: sfp_mul_const_rescale(_add), no weighted-sum launch
    // and no temporary (SFHE_CONST_TERMS=0, read per call: as a sum, then a
    // rescale; the same integers).
    // Engine extension: terms[j] = (c_j, at_j): c_j * x at level at_j (> x's
    // level), each what LinearWSumRescale({x}, {c_j}, at_j - 1) gives.  Up to
    // SFP_MAX_CONST_TERMS of them share one inverse and one forward NTT launch
    // pair (sfp_const_terms_rescale) where the backend has that prim and x's
    // rows are not dealt over ranks; else (the C oracle, SFHE_CONST_TERMS=0)
    // they are formed one by one.
    std::vector<Ciphertext<DCRTPoly>> ConstTermsRescale(const Ciphertext<DCRTPoly>& x,
                                                        const std::vector<std::pair<double, uint32_t>>& terms);
    // Engine extension: nout weighted sums of the same inputs in one pass
    // (one multi-output kernel + one batched rescale); w[o] has nin weights.
    std::vector<Ciphertext<DCRTPoly>> LinearWSumRescaleMulti(
        const std::vector<const uint64_t*>& in0, const std::vector<const uint64_t*>& in1,
        const std::vector<std::vector<double>>& w, uint32_t level, uint32_t slots,
        const std::vector<double>* inScale = nullptr);
    // ... with output o's constant term constants[o]: *constantsAdded = true
    // when the rescale's last pass added them all, false when none was added
    // (the caller then adds them: EvalAdd(out[o], constants[o]))
    std::vector<Ciphertext<DCRTPoly>> LinearWSumRescaleMulti(
        const std::vector<const uint64_t*>& in0, const std::vector<const uint64_t*>& in1,
        const std::vector<std::vector<double>>& w, uint32_t level, uint32_t slots,
        const std::vector<double>* inScale, const std::vector<double>* constants, bool* constantsAdded);
    // Engine internal (SFHE_PS_DEBUG): sums the backend has folded into a
    // producing op's last pass so far -- ciphertext addends, constants -- and
    // weighted sums whose two polynomials went out as one launch
    void FusedSumCounts(uint64_t* sums, uint64_t* consts, uint64_t* pairedWsums) const;
    // Wait for all device work; throws on an asynchronous device error.
    void Synchronize();
    // Lazy rescaling: compute / rescale ct's rows now (canonical form at its
    // level); every evaluator entry point does this for inputs it cannot take
    // unrescaled.  Needed only before reading c0 / c1 directly.
    void Settle(const Ciphertext<DCRTPoly>& ct);
    // Engine extension: independent work on concurrent lanes (HIP streams).
    // ForkLanes(k) orders lanes 1..k-1 after everything issued so far on lane
    // 0; SetLane(i) routes the following operations to lane i; JoinLanes()
    // orders lane 0 after all of them.  Objects created on a lane may be
    // read on other lanes only after the join.
    int LaneCount() const;
    // Limb sharding (engine extension): this process holds the
    // RNS limbs i with i % world == rank of every ciphertext; levels with at
    // most ShardTailLimbs() limbs run replicated on every rank (SFHE_SHARD_TAIL,
    // default 16); every rank keeps its slice of the switching keys (the rows
    // of those levels, of its own dealt primes and the P rows).  Call before key
    // generation, with the device communicator set up (C ABI sfhe_comm_*).
    // shardAtOne: a one-rank communicator still takes the sharded code path
    // (single-GPU validation of the exchanges).  Results are bit-identical
    // to the unsharded context.
    void EnableSharding(int rank, int world, bool shardAtOne = false);
    int ShardRank() const;
    int ShardWorld() const;
    bool IsSharded() const;
    uint32_t ShardTailLimbs() const;
    // rows per digit part of this rank's switching keys: Lq + K for whole
    // keys, fewer for a sliced key (sharded, world > 1; SFHE_KEY_SLICE=0: whole)
    uint32_t SwitchKeyRows() const;
    // Batch groups (engine extension): the sort's independent
    // batches are split over `groups` GPU groups, this rank in group `group`
    // (each group limb-sharded or not).  The device's group communicator
    // (C ABI sfhe_groups_*) joins the ranks holding the same rows of
    // different groups.  GatherGroups(ct) settles ct and all-gathers it over
    // that communicator: every group's ciphertext, group order (collective:
    // every rank calls it in the same program order).
    // gatherAtOne: a one-group communicator still routes the parts through
    // GatherGroups (single-GPU validation of the collective, as shardAtOne).
    void EnableBatchGroups(int group, int groups, bool gatherAtOne = false);
    int BatchGroup() const;
    int BatchGroups() const;
    bool BatchGather() const;  // groups > 1, or gatherAtOne
    std::vector<Ciphertext<DCRTPoly>> GatherGroups(const Ciphertext<DCRTPoly>& ct);
    // Engine internal (raw-row consumers: the weighted sums): ct's (c0, c1)
    // rows, Settle()d, as valid at `level`'s limb count -- gathered into a
    // buffer appended to `keep` when ct's rows are dealt over the ranks but
    // that count falls in the replicated tail.
    void RowsAt(const Ciphertext<DCRTPoly>& ct, uint32_t level, const uint64_t** c0, const uint64_t** c1,
                std::vector<DeviceBufferPtr>& keep);
    // raw residues [c0 rows][c1 rows] of every limb, natural order (collective when sharded)
    void DownloadRows(const Ciphertext<DCRTPoly>& ct, uint64_t* out);
    // stacked: the region's lanes are issued as stacked launches (prims.h
    // sfp_stack_begin): identical ops of different lanes become one launch;
    // JoinLanes issues them.  For lanes that run the same op sequence.
    void ForkLanes(int count, bool stacked = false);
    // Batched ops (prims.h sfp_batch_*): between BeginBatch(count) and
    // EndBatch(), op i is issued after BatchLane(i); the ops must be
    // independent, their identical launches run merged, everything is issued
    // on this lane at EndBatch (blocks freed meanwhile are reused after it).
    // BeginBatch returns false (the ops simply run) where batching is off.
    // (BeginBatch holds the context's op lock until EndBatch; see BatchScope)
    bool BeginBatch(uint32_t count);
    void BatchLane(uint32_t i);
    void EndBatch();
    uint32_t BatchWidth() const;  // ops per batch (SFHE_BATCH_WIDTH)
    // Engine extension: run the deferred ops of several independent
    // ciphertexts as batched ops, one virtual lane each -- cts[i] in the form
    // its consumer will take: pending rows where pendingOk[i], canonical
    // otherwise (exactly what the consumer's own materialisation would run:
    // the same values).  A batch is a run of up to BatchWidth() ops of one
    // level, one kind (products, plaintext products, ...) and one form;
    // whatever is alone of its kind, and a rescale of rows already pending,
    // runs unbatched.  Only batches of canonical ciphertext products are
    // exercised so far (the sign's waves).  Where batching is unavailable (SFHE_BATCH=0, a sharded level,
    // an open batch or stacked region, a backend that never merges) the ops
    // run one after the other.
    void MaterializeMany(const std::vector<Ciphertext<DCRTPoly>>& cts, const std::vector<char>& pendingOk);
    void SetLane(int lane);
    void JoinLanes();
    // Plaintext-encoding cache across calls (default on); see DESIGN.md.
    void SetPlaintextCache(bool on);
    // Operation counters (for the roofline byte model).
    struct OpStats {
        uint64_t keyswitch = 0, rescale = 0, tensor = 0, ptmult = 0, constmult = 0, add = 0,
                 automorph = 0, ntt_limbs = 0, wsum_terms = 0;
        uint64_t dev_encodes = 0, host_encodes = 0;  // plaintext encodings on the device / host
        uint64_t dev_decodes = 0, host_decodes = 0;  // decrypted ciphertexts decoded on the device / host
        uint64_t dev_samples = 0, host_samples = 0;  // small polynomials (ternary, error) sampled on the device / host
        double algo_bytes = 0.0;  // SURVEY.md §8(d) byte model
        uint64_t pool_bytes = 0;  // device memory held by the context's pool (live + free blocks)
        uint64_t tie_fused = 0, tie_composed = 0;  // EvalTieTerm tensors in one launch / composed of generic prims
        // constant terms c x (one-input weighted sums): inside a multi-term launch
        // (sfp_const_terms_rescale) / as one fused constant rescale / as a weighted sum, then a rescale
        uint64_t const_merged = 0, const_single = 0, const_composed = 0;
        // multi-column placements: indicators evaluated, columns they served, giant-step sums formed
        // by sfp_mac_plain2_cols / left to the per-column path
        uint64_t place_hits = 0, place_columns = 0, place_fused = 0, place_composed = 0;
        // selections: indicator batches run; EvalRotateFold calls whose inner products were one
        // launch (sfp_ks_inner_aut_sum) / composed of the generic prims
        uint64_t select_batches = 0, fold_fused = 0, fold_composed = 0;
        // multi-column selections: columns served; EvalRotateFoldMany's launches of
        // sfp_ks_inner_aut_sum_cols / columns it passed to EvalRotateFold
        uint64_t select_columns = 0, fold_cols_fused = 0, fold_cols_composed = 0;
        uint64_t lex_fused = 0, lex_composed = 0;  // EvalLexStep tensors in one launch / composed of generic prims
        uint64_t dot_fused = 0, dot_composed = 0;  // EvalMultSum2 as one fused chain / composed of generic prims
        uint64_t sumn_fused = 0, sumn_composed = 0;  // EvalMultSum(Many) ops likewise (EvalMultSum2's not included)
        // EvalMultSumMany's runs of one level and term count (each goes out as one batch), and
        // remainder chains of the Chebyshev evaluator that fell outside EvalMultSum's conditions
        // and ran as separate products and sums
        uint64_t sumn_batches = 0, sumn_fallbacks = 0;
        uint64_t gate_fused = 0, gate_composed = 0;  // EvalGateSumMany calls: tensors fused / composed of generic prims
        uint64_t weight_fused = 0, weight_composed = 0;  // EvalWeightSumMany calls likewise
        uint64_t or_fused = 0, or_composed = 0;  // EvalGateOr calls: tensor in one launch / composed of generic prims
    };
    OpStats GetOpStats() const;
    void ResetOpStats();
    // Engine extension: hipGraph capture of a data-independent op sequence
    // (the sort's steady state).  BeginCapture() drains the device and starts
    // recording (false: the backend has no graphs -- run eagerly);
    // EndCapture(keep) finishes it: nullptr if the region could not be
    // captured (a host synchronisation inside; the reason is in the log),
    // otherwise a graph that owns every pool block the region allocated plus
    // `keep` (the region's result, read after each launch).  Launch() replays
    // it on the current lane, stream-ordered with everything else.
    struct CapturedGraph;
    bool BeginCapture();
    std::shared_ptr<CapturedGraph> EndCapture(const Ciphertext<DCRTPoly>& keep);
    void Launch(const std::shared_ptr<CapturedGraph>& g);
    // Engine internal: destroy g's executable graph and hand its pool blocks
    // back now (a graph the context itself holds, at context destruction,
    // when its weak context reference no longer locks)
    void ReleaseGraph(CapturedGraph& g);
    // contexts alive in this process (diagnostics: a context kept alive by a
    // reference cycle keeps its device memory)
    static int LiveContexts();
    // ... for every bootstrap replay graph (bootstrap.cpp)
    void releaseBootstrapGraphs();
    size_t GraphNodes(const std::shared_ptr<CapturedGraph>& g) const;
    // the graph's NTT kernels replayed alone (sfp_graph_family_time)
    // (family: prims.h SFP_FAM_*, SFP_FAM_COUNT = the other kernels, SFP_FAM_ALL = all)
    bool GraphFamilyTime(const std::shared_ptr<CapturedGraph>& g, uint32_t family, int reps, double* ms,
                         uint64_t* launches, double* bytes);
    // dst's rows (same level) overwritten with src's: refills a graph's input
    void CopyCiphertextInto(const Ciphertext<DCRTPoly>& dst, const Ciphertext<DCRTPoly>& src);

  private:
    bool multAddFusable(const Ciphertext<DCRTPoly>& a, const Ciphertext<DCRTPoly>& b, const MultAddend& add) const;
    // the shared body of EvalMultMany (adds null) and EvalMultManyAdd; who: the caller, for messages
    std::vector<Ciphertext<DCRTPoly>> multMany(const std::vector<Ciphertext<DCRTPoly>>& a,
                                               const std::vector<Ciphertext<DCRTPoly>>& b,
                                               const std::vector<MultAddend>* adds, const char* who);
    std::unique_ptr<SfheContextState> st;
    uint32_t enabled = 0;
    BootstrapTap bootTap;
    friend class SfheInternal;
};

// A batch of independent ops (CryptoContextImpl::BeginBatch) for one scope:
// ends the batch on every exit path.  count < 2: no batch, the ops just run.
class BatchScope {
  public:
    BatchScope(CryptoContextImpl<DCRTPoly>* cc, uint32_t count)
        : cc_(cc), on_(count > 1 && cc->BeginBatch(count)) {}
    ~BatchScope() {
        if (on_) cc_->EndBatch();
    }
    BatchScope(const BatchScope&) = delete;
    BatchScope& operator=(const BatchScope&) = delete;
    explicit operator bool() const { return on_; }
    void lane(uint32_t i) {
        if (on_) cc_->BatchLane(i);
    }
    void end() {  // before the scope's end
        if (on_) cc_->EndBatch();
        on_ = false;
    }

  private:
    CryptoContextImpl<DCRTPoly>* cc_;
    bool on_;
};

// Registers the context for key deserialization (Deserialize*Key below find
// their context by its parameter fingerprint, as OpenFHE's static key maps do).
void RegisterCryptoContext(const CryptoContext<DCRTPoly>& cc);

// ---------------------------------------------------------------------------
// Layout stamp: the ABI handshake between a caller and the library.  Callers
// compile the classes above into their own objects (inline accessors, field
// reads, make_shared), so a caller built against headers other than the
// library's reads and writes them at the wrong offsets: silent heap
// corruption (two reference-harness programs built against older headers
// aborted in malloc this way).  The stamp hashes the version, the
// size and alignment of every class defined here, the offset of every public
// field and the sizes of the standard-library types inside them (a different
// libstdc++ ABI or _GLIBCXX_DEBUG changes those); GenCryptoContext hands the
// caller's stamp to the library, which throws OpenFHEException on a mismatch.
// SFHE_LAYOUT_SALT exists only for the test that builds a deliberately
// mismatched caller (tests/test_abi_stamp.py).
#define SFHE_FACADE_ABI_VERSION 17
#ifndef SFHE_LAYOUT_SALT
#define SFHE_LAYOUT_SALT 0
#endif
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Winvalid-offsetof"
inline uint64_t SfheFacadeLayout() {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t x) { h = (h ^ x) * 1099511628211ull; };
    using Ct = CiphertextImpl<DCRTPoly>;
    using Pk = PublicKeyImpl<DCRTPoly>;
    using Sk = PrivateKeyImpl<DCRTPoly>;
    using Cc = CryptoContextImpl<DCRTPoly>;
    const uint64_t v[] = {
        SFHE_FACADE_ABI_VERSION, SFHE_LAYOUT_SALT,
        sizeof(std::string), sizeof(std::mutex), sizeof(std::shared_ptr<int>), sizeof(std::vector<int>),
        sizeof(std::map<int, int>), sizeof(std::set<int>), sizeof(std::function<void()>), sizeof(std::complex<double>),
        sizeof(CCParams<CryptoContextCKKSRNS>), alignof(CCParams<CryptoContextCKKSRNS>),
        sizeof(EncodingParamsImpl), sizeof(KeyPair<DCRTPoly>),
        sizeof(PlaintextImpl), alignof(PlaintextImpl), offsetof(PlaintextImpl, values), offsetof(PlaintextImpl, slots),
        offsetof(PlaintextImpl, level), offsetof(PlaintextImpl, length), offsetof(PlaintextImpl, logPrecision),
        offsetof(PlaintextImpl, logError), offsetof(PlaintextImpl, realCache), offsetof(PlaintextImpl, encoded),
        offsetof(PlaintextImpl, encMutex),
        sizeof(Ct), alignof(Ct), offsetof(Ct, cc), offsetof(Ct, buf), offsetof(Ct, c0), offsetof(Ct, c1),
        offsetof(Ct, level), offsetof(Ct, slots), offsetof(Ct, scale), offsetof(Ct, def), offsetof(Ct, pend),
        offsetof(Ct, undo), sizeof(Ct::CaptureUndo),
        sizeof(Pk), offsetof(Pk, b), offsetof(Pk, a), offsetof(Pk, cc), offsetof(Pk, tag),
        sizeof(Sk), offsetof(Sk, s), offsetof(Sk, ternary), offsetof(Sk, cc), offsetof(Sk, tag),
        sizeof(FastRotationPrecomp), offsetof(FastRotationPrecomp, ext), offsetof(FastRotationPrecomp, level),
        offsetof(FastRotationPrecomp, pend), offsetof(FastRotationPrecomp, beta), offsetof(FastRotationPrecomp, stride),
        offsetof(FastRotationPrecomp, pinBuf), offsetof(FastRotationPrecomp, pinC0),
        sizeof(Cc), alignof(Cc), sizeof(Cc::OpStats), sizeof(Cc::BootstrapTap),
    };
    for (uint64_t x : v) mix(x);
    return h;
}
#pragma GCC diagnostic pop
// Library side: throws OpenFHEException unless callerStamp is the library's
// own SfheFacadeLayout() (context.cpp).
void SfheCheckLayout(uint64_t callerStamp);

inline CryptoContext<DCRTPoly> GenCryptoContext(const CCParams<CryptoContextCKKSRNS>& p) {
    SfheCheckLayout(SfheFacadeLayout());
    auto cc = std::make_shared<CryptoContextImpl<DCRTPoly>>(p);
    RegisterCryptoContext(cc);
    return cc;
}

// ---------------------------------------------------------------------------
// Serialization (OpenFHE utils/serial.h surface the reference's src/sort.h:31-102
// uses).  Format: the engine's own binary records (magic "SFHE", a type
// tag, the context's parameter fingerprint, raw residues) -- OpenFHE's
// cereal BINARY layout cannot be reproduced without OpenFHE (SURVEY §8(f)
// row 4), so files round-trip between processes of this engine, not with
// OpenFHE.  SerType::JSON is rejected.
class Serial {
  public:
    static bool Serialize(const CryptoContext<DCRTPoly>& cc, std::ostream& os, SerType::Kind k);
    static bool Deserialize(CryptoContext<DCRTPoly>& cc, std::istream& is, SerType::Kind k);
    static bool Serialize(const PublicKey<DCRTPoly>& pk, std::ostream& os, SerType::Kind k);
    static bool Deserialize(PublicKey<DCRTPoly>& pk, std::istream& is, SerType::Kind k);
    static bool Serialize(const PrivateKey<DCRTPoly>& sk, std::ostream& os, SerType::Kind k);
    static bool Deserialize(PrivateKey<DCRTPoly>& sk, std::istream& is, SerType::Kind k);
    static bool Serialize(const Ciphertext<DCRTPoly>& ct, std::ostream& os, SerType::Kind k);
    static bool Deserialize(Ciphertext<DCRTPoly>& ct, std::istream& is, SerType::Kind k);

    template <class T>
    static bool SerializeToFile(const std::string& path, const T& obj, SerType::Kind k) {
        std::ofstream f(path, std::ios::out | std::ios::binary | std::ios::trunc);
        if (!f.is_open()) return false;
        return Serialize(obj, f, k) && f.good();
    }
    template <class T>
    static bool DeserializeFromFile(const std::string& path, T& obj, SerType::Kind k) {
        std::ifstream f(path, std::ios::in | std::ios::binary);
        if (!f.is_open()) return false;
        return Deserialize(obj, f, k);
    }
};

template <class E>
class CryptoContextFactory {
  public:
    static void ReleaseAllContexts() {}
};

// OpenFHE math/chebyshev.h: Chebyshev interpolation coefficients (c0/2
// convention) of f on [a,b] at `degree` Chebyshev nodes.
// body(i) for i < count over the host's cores (engine utility for the
// O(degree^2) coefficient transforms: each index is computed alone, so the
// results do not depend on the thread count)
template <class F>
void ParallelFor(size_t count, F&& body, size_t minCount = 64) {
    const size_t T = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(std::thread::hardware_concurrency(), 16), count));
    if (T == 1 || count < minCount) {
        for (size_t i = 0; i < count; ++i) body(i);
        return;
    }
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            for (size_t i = t; i < count; i += T) body(i);
        });
    for (auto& x : th) x.join();
}

std::vector<double> EvalChebyshevCoefficients(std::function<double(double)> func, double a,
                                              double b, uint32_t degree);

// OpenFHE's depth of EvalChebyshevSeriesPS for a polynomial of this degree
// (input already in [-1,1]).
uint32_t ChebyshevPSDepth(uint32_t degree);

}  // namespace lbcrypto

// Reference tests print vectors with operator<< (DirectSortTest.cpp:148,151).
template <class T>
inline std::ostream& operator<<(std::ostream& os, const std::vector<T>& v) {
    os << "[";
    for (size_t i = 0; i < v.size(); ++i) os << (i ? ", " : "") << v[i];
    return os << "]";
}

// Vectors of doubles (the debug prints of 32 768-slot decryptions): on a
// stream with the default float format (%g, precision 6, classic locale, no
// width) each value is formatted with std::to_chars -- the same characters
// as the stream would write (checked on 2 M random values, NaN, infinities,
// signed zeros, subnormals), about 4x faster -- and the text written at once.
inline std::ostream& operator<<(std::ostream& os, const std::vector<double>& v) {
    const auto fl = os.flags();
    const bool plain = (fl & (std::ios_base::floatfield | std::ios_base::showpos | std::ios_base::showpoint |
                              std::ios_base::uppercase)) == 0 &&
                       os.precision() == 6 && os.width() == 0 && os.getloc() == std::locale::classic();
    if (!plain) {
        os << "[";
        for (size_t i = 0; i < v.size(); ++i) os << (i ? ", " : "") << v[i];
        return os << "]";
    }
    // (long vectors: 16 slices formatted on host threads, written in order)
    const size_t T = v.size() >= 4096 ? 16 : 1, per = (v.size() + T - 1) / T;
    std::vector<std::string> parts(T);
    lbcrypto::ParallelFor(T, [&](size_t p) {
        std::string& out = parts[p];
        out.reserve(per * 14 + 2);
        char b[64];
        for (size_t i = p * per; i < std::min(v.size(), (p + 1) * per); ++i) {
            if (i) out += ", ";
            const auto r = std::to_chars(b, b + sizeof b, v[i], std::chars_format::general, 6);
            out.append(b, r.ptr);
        }
    }, 1);
    os.put('[');
    for (const auto& part : parts) os.write(part.data(), (std::streamsize)part.size());
    return os.put(']');
}
