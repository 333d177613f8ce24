// Composite sign polynomials on the device engine.
//
// Reference: src/sign.cpp:9-60 (CompositeSign<3>), :62-158
// (CompositeSign<4>), :160-185 (composition with lazy bootstrap),
// :635-651 (dispatcher).  The polynomials are the published ones
// (Cheon-Kim-Kim 2019); the evaluation order keeps the reference's depth:
// every odd polynomial of degree 2^k - 1 costs exactly k levels because the
// coefficient multiplications happen at depth 1.
#include "sign.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <vector>

using namespace lbcrypto;

namespace {

using Ct = Ciphertext<DCRTPoly>;

// c x at level `at` (> x's level)
Ct constTermAt(const CryptoContext<DCRTPoly>& cc, const Ct& x, double c, uint32_t at) {
    const uint64_t *r0, *r1;
    std::vector<DeviceBufferPtr> keep;
    cc->RowsAt(x, at - 1, &r0, &r1, keep);  // settled (and gathered into a replicated tail)
    const std::vector<const uint64_t*> i0{r0}, i1{r1};
    const std::vector<double> w{c}, sc{x->scale};
    return cc->LinearWSumRescale(i0, i1, w, at - 1, x->GetSlots(), &sc);
}

// SFHE_SIGN_DOT=0 (read per call): a node and its `lo` child keep their two
// separate products (see OddPoly).
bool signDot() {
    const char* v = std::getenv("SFHE_SIGN_DOT");
    return !v || *v != '0';
}

// sum_{i} c[i] x^(2i+1) for c.size() == 2^(k-1) odd coefficients, depth k:
//   P(x) = A(x) + B(x) * x^(2^(k-1)),  A,B of half the degree.
// pw[j] holds x^(2^(j+1)) (x^2, x^4, x^8, ...).
//
// Every term lands directly at the level its sum works at, so no partial sum
// is level-adjusted: B is formed at the level just above the product's, A at
// the product's level, and a coefficient times x at whatever level it is
// wanted, as one weighted sum that folds the scale into its integer weight
// (one rescale, like EvalMult(x, c), but at any level below x's).  Only a
// power x^(2^j) may need aligning, once per level (memo).  Degree 7: 10
// rescales instead of 12 (4 coefficient products, 5 ciphertext products, x^2
// aligned once); same depth and polynomial.
//
// Paired products: where a node's `lo` child A is itself a product node,
//   A + B x^(2^j) = A.lo + A.hi x^(2^j') + B x^(2^j),
// both products work at the node's level (`want` lands A there: operands at
// Lp - 1) and are only added, so they go out as ONE sum of two products
// (EvalMultSum2: one relinearisation, ModDown and rescale) with A.lo as its
// addend.  Degree 7 pairs at the root ((c3 x) x^2 with B x^4, addend c1 x);
// degree 15 at the root and at the root's `hi` child.  A.lo and B are whole
// nodes of their own (and pair again where the rule holds).
struct OddPoly {
    const CryptoContext<DCRTPoly>& cc;
    const Ct& x;
    const std::vector<Ct>& pw;
    std::map<std::pair<size_t, uint32_t>, Ct> aligned;
    const bool dot = signDot();

    Ct constAt(double c, uint32_t at) { return constTermAt(cc, x, c, at); }
    const Ct& power(size_t j, uint32_t level) {
        if (pw[j]->GetLevel() >= level) return pw[j];
        auto key = std::make_pair(j, level);
        auto it = aligned.find(key);
        if (it != aligned.end()) return it->second;
        return aligned[key] = cc->AdjustLevel(pw[j], level);
    }
    static size_t powIndex(size_t half) {
        size_t j = 0;
        while ((size_t)2 << j < 2 * half) ++j;  // x^(2*half) = pw[j]
        return j;
    }
    // level eval(c, cnt, 0) reaches
    uint32_t natural(size_t cnt) const {
        if (cnt == 1) return x->GetLevel() + 1;
        const size_t half = cnt / 2;
        return std::max(natural(half), pw[powIndex(half)]->GetLevel()) + 1;
    }
    Ct eval(const double* c, size_t cnt, uint32_t want) {
        if (cnt == 1) return constAt(c[0], std::max(x->GetLevel() + 1, want));
        const size_t half = cnt / 2, j = powIndex(half);
        const uint32_t Lp = std::max(std::max(natural(half), pw[j]->GetLevel()) + 1, want);
        Ct hi = eval(c + half, half, Lp - 1);
        if (dot && half > 1) {
            const size_t half2 = half / 2, j2 = powIndex(half2);
            if (std::max(std::max(natural(half2), pw[j2]->GetLevel()) + 1, Lp) == Lp) {  // (the child's level)
                Ct hi2 = eval(c + half2, half2, Lp - 1);
                Ct lolo = eval(c, half2, Lp);
                const Ct p1 = power(j, Lp - 1), p2 = power(j2, Lp - 1);
                for (const Ct& o : {hi, p1, hi2, p2, lolo}) cc->Settle(o);
                return cc->EvalMultSum2(hi, p1, hi2, p2, lolo);
            }
        }
        Ct prod = cc->EvalMult(hi, power(j, Lp - 1));
        Ct lo = eval(c, half, Lp);
        return cc->EvalAdd(lo, prod);
    }
};

// SFHE_SIGN_BATCH=0: OddPoly::eval's issue order (every op alone, when its
// consumer asks for it).  Read once.
bool signBatch() {
    static const bool on = [] {
        const char* v = std::getenv("SFHE_SIGN_BATCH");
        return !v || *v != '0';
    }();
    return on;
}

// OddPoly's tree -- the same nodes, levels, coefficient terms, aligned powers
// and sums -- issued wave by wave: the tree is built first (no device work),
// then every wave's products -- the next power x^(2^j) and the nodes'
// B(x) * x^(2^j) whose operands exist (degree 7: x^2 | x^4, (c3 x) x^2 |
// B x^4, (c1 x) x^2) -- go out through MaterializeMany, which batches those
// of one level, so their identical launches merge.  The coefficient terms
// (they depend on x alone: all after the first wave, as one multi-term
// constant rescale, ConstTermsRescale) and the alignment of a power (after the
// wave that made it) follow the wave's products outside any batch: batching
// them as well gave wrong rows in larger sorts.
// A node's sum follows the wave of its product, as before.  Every op sees
// the operands it saw in OddPoly::eval, in the same form: a product's sum
// partner `lo` is canonical at the product's own level (`want` lands it
// there), so the sum takes the product's canonical form there as well.
// A paired node (OddPoly: its `lo` child is a product node) issues its own and
// the child's product as one EvalMultSum2 once the operands of both and the
// child's `lo` exist; the child forms no product or sum of its own.
struct OddPolyWaves {
    const CryptoContext<DCRTPoly>& cc;
    const Ct& x;
    const uint32_t L;  // x's level; x^(2^(j+1)) is at L + j + 1
    struct Node {
        const double* c;
        size_t cnt, j;
        uint32_t Lp;  // a leaf's level / the level of the node's product and sum
        int hi, lo;
        Ct prod, out;
        int pair = -1;          // the `lo` child whose product rides in this node's EvalMultSum2
        bool absorbed = false;  // such a child
    };
    std::vector<Node> nodes;
    std::vector<Ct> pw;
    std::map<std::pair<size_t, uint32_t>, Ct> aligned;
    const bool dot = signDot();

    uint32_t pwLevel(size_t j) const { return L + 1 + (uint32_t)j; }
    uint32_t natural(size_t cnt) const {
        if (cnt == 1) return L + 1;
        const size_t half = cnt / 2;
        return std::max(natural(half), pwLevel(OddPoly::powIndex(half))) + 1;
    }
    // OddPoly::eval(c, cnt, want) as a node (children first)
    int build(const double* c, size_t cnt, uint32_t want) {
        Node nd{c, cnt, 0, 0, -1, -1, nullptr, nullptr};
        if (cnt == 1) {
            nd.Lp = std::max(L + 1, want);
        } else {
            const size_t half = cnt / 2;
            nd.j = OddPoly::powIndex(half);
            nd.Lp = std::max(std::max(natural(half), pwLevel(nd.j)) + 1, want);
            nd.hi = build(c + half, half, nd.Lp - 1);
            nd.lo = build(c, half, nd.Lp);
            if (dot && nodes[nd.lo].cnt > 1 && nodes[nd.lo].Lp == nd.Lp) {
                nd.pair = nd.lo;
                Node& ch = nodes[nd.lo];
                ch.absorbed = true;
                if (ch.pair >= 0) {  // (its own `lo` is this node's addend: a whole node again)
                    nodes[ch.pair].absorbed = false;
                    ch.pair = -1;
                }
            }
        }
        nodes.push_back(nd);
        return (int)nodes.size() - 1;
    }
    Ct run(const std::vector<double>& c) {
        const int root = build(c.data(), c.size(), 0);
        size_t npw = 1;  // even powers x^2, x^4, ... up to x^(cnt)
        for (size_t p = 4; p < 2 * c.size(); p *= 2) ++npw;
        cc->Settle(x);
        while (!nodes[root].out) {
            std::vector<Ct> prods;
            const size_t ready = pw.size();  // the powers earlier waves made
            if (pw.size() < npw) {
                pw.push_back(cc->EvalSquare(pw.empty() ? x : pw.back()));
                prods.push_back(pw.back());
            }
            // the node products whose operands exist; a power made by an
            // earlier wave that a node wants at a higher level is aligned after
            // this wave's products (once per level), for the next wave
            std::vector<std::pair<size_t, uint32_t>> align;
            // a node's power at its operand level; null, with the alignment asked for, while it is not there
            auto powerOf = [&](const Node& nd) -> const Ct* {
                if (nd.j >= ready) return nullptr;
                if (pwLevel(nd.j) >= nd.Lp - 1) return &pw[nd.j];
                const auto key = std::make_pair(nd.j, nd.Lp - 1);
                auto it = aligned.find(key);
                if (it != aligned.end()) return &it->second;
                if (std::find(align.begin(), align.end(), key) == align.end()) align.push_back(key);
                return nullptr;
            };
            size_t dots = 0;
            for (Node& nd : nodes) {
                if (nd.cnt == 1 || nd.prod || nd.out || nd.absorbed) continue;
                const Ct* power = powerOf(nd);
                if (nd.pair >= 0) {  // both products and the child's `lo` in one op
                    const Node& ch = nodes[nd.pair];
                    const Ct* power2 = powerOf(ch);
                    if (!power || !power2 || !nodes[nd.hi].out || !nodes[ch.hi].out || !nodes[ch.lo].out) continue;
                    nd.out = cc->EvalMultSum2(nodes[nd.hi].out, *power, nodes[ch.hi].out, *power2, nodes[ch.lo].out);
                    ++dots;
                    continue;
                }
                if (!power || !nodes[nd.hi].out) continue;
                nd.prod = cc->EvalMult(nodes[nd.hi].out, *power);
                prods.push_back(nd.prod);
            }
            const bool first = ready == 0;
            if (prods.empty() && align.empty() && !first && !dots)
                throw OpenFHEException("internal: odd-polynomial wave evaluation stalled");
            cc->MaterializeMany(prods, std::vector<char>(prods.size(), 0));
            if (first) {
                // the coefficient terms need x alone (held until their sums: a
                // few rows longer than before): constant rescales of one input,
                // up to four in one launch pair per direction (ConstTermsRescale;
                // no batch is involved)
                std::vector<std::pair<double, uint32_t>> terms;
                for (const Node& nd : nodes)
                    if (nd.cnt == 1) terms.emplace_back(nd.c[0], nd.Lp);
                const auto cts = cc->ConstTermsRescale(x, terms);
                size_t t = 0;
                for (Node& nd : nodes)
                    if (nd.cnt == 1) nd.out = cts[t++];
            }
            for (const auto& key : align) aligned[key] = cc->AdjustLevel(pw[key.first], key.second);
            for (Node& nd : nodes)
                if (nd.cnt > 1 && !nd.out && nd.prod && nodes[nd.lo].out) nd.out = cc->EvalAdd(nodes[nd.lo].out, nd.prod);
        }
        return nodes[root].out;
    }
};

Ct oddPolyFull(const CryptoContext<DCRTPoly>& cc, const Ct& x, const std::vector<double>& c) {
    if (signBatch() && c.size() > 1) {
        OddPolyWaves w{cc, x, x->GetLevel(), {}, {}, {}};
        return w.run(c);
    }
    // even powers x^2, x^4, ... up to x^(cnt)
    std::vector<Ct> pw;
    pw.push_back(cc->EvalSquare(x));
    for (size_t p = 4; p < 2 * c.size(); p *= 2) pw.push_back(cc->EvalSquare(pw.back()));
    OddPoly op{cc, x, pw, {}};
    return op.eval(c.data(), c.size(), 0);
}

template <int n>
struct CompositePolys;

// g_3(x) = (4589x - 16577x^3 + 25614x^5 - 12860x^7) / 2^10
// f_3(x) = (35x - 35x^3 + 21x^5 - 5x^7) / 2^4
template <>
struct CompositePolys<3> {
    static constexpr int g_depth = 3, f_depth = 3;
    static Ct g(const Ct& x, const CryptoContext<DCRTPoly>& cc) {
        static const std::vector<double> c = {4589.0 / 1024, -16577.0 / 1024, 25614.0 / 1024,
                                              -12860.0 / 1024};
        return oddPolyFull(cc, x, c);
    }
    static Ct f(const Ct& x, const CryptoContext<DCRTPoly>& cc) {
        static const std::vector<double> c = {35.0 / 16, -35.0 / 16, 21.0 / 16, -5.0 / 16};
        return oddPolyFull(cc, x, c);
    }
};

// g_4: degree-27 Chebyshev series (depth 5); f_4: odd degree-15 (depth 4).
template <>
struct CompositePolys<4> {
    static constexpr int g_depth = 4, f_depth = 4;
    static Ct g(const Ct& x, const CryptoContext<DCRTPoly>& cc) {
        static const std::vector<double> cheb = {
            0.0, 1.077117252745569,    0.0, -0.36166113998402755,
            0.0, 0.2137420717859748,   0.0, -0.15635204788780485,
            0.0, 0.11749645501187332,  0.0, -0.10074154666447852,
            0.0, 0.08002086947825496,  0.0, -0.07533558758484624,
            0.0, 0.059514472116534836, 0.0, -0.06146663712787884,
            0.0, 0.04570084927999001,  0.0, -0.05403683682999072,
            0.0, 0.03364293851188723,  0.0, -0.054459493266273494};
        return cc->EvalChebyshevSeriesPS(x, cheb, -1, 1);
    }
    static Ct f(const Ct& x, const CryptoContext<DCRTPoly>& cc) {
        static const std::vector<double> c = {3.14208984375,  -7.33154296875, 13.19677734375,
                                              -15.71044921875, 12.21923828125, -5.99853515625,
                                              1.69189453125,  -0.20947265625};
        return oddPolyFull(cc, x, c);
    }
};

}  // namespace

template <int n>
Ciphertext<DCRTPoly> compositeSign(Ciphertext<DCRTPoly> x, CryptoContext<DCRTPoly> cc,
                                   const SignConfig& Cfg) {
    // Bootstrap before a polynomial that would not fit the remaining budget
    // (never triggers at the default multDepth = 100).
    auto refresh = [&](Ct& c, int need) {
        if (Cfg.multDepth - (int)c->GetLevel() < need + 2) c = cc->EvalBootstrap(c);
    };
    // g is applied max(dg, 1) times: the reference applies it once before
    // its loop over i = 1 .. dg-1 (src/sign.cpp:173-178), so dg = 0 still
    // evaluates g once (SignTest's CompositeSignTest relies on it).
    Ct y = x;
    const int gCount = Cfg.compos.dg > 1 ? Cfg.compos.dg : 1;
    for (int i = 0; i < gCount; ++i) {
        refresh(y, CompositePolys<n>::g_depth);
        y = CompositePolys<n>::g(y, cc);
    }
    for (int i = 0; i < Cfg.compos.df; ++i) {
        refresh(y, CompositePolys<n>::f_depth);
        y = CompositePolys<n>::f(y, cc);
    }
    return y;
}

template Ciphertext<DCRTPoly> compositeSign<3>(Ciphertext<DCRTPoly>, CryptoContext<DCRTPoly>,
                                               const SignConfig&);
template Ciphertext<DCRTPoly> compositeSign<4>(Ciphertext<DCRTPoly>, CryptoContext<DCRTPoly>,
                                               const SignConfig&);

Ciphertext<DCRTPoly> sign(Ciphertext<DCRTPoly> x, CryptoContext<DCRTPoly> cc, SignFunc func,
                          const SignConfig& Cfg) {
    if (func == SignFunc::CompositeSign) {
        if (Cfg.compos.n == 3) return compositeSign<3>(x, cc, Cfg);
        if (Cfg.compos.n == 4) return compositeSign<4>(x, cc, Cfg);
    }
    // SignumPolycircuit / Tanh / NaiveDiscrete (and the reference's
    // fall-through for other n, sign.cpp:638-645) are outside the hot path.
    throw OpenFHEException("sign: only SignFunc::CompositeSign with n in {3,4} is implemented");
}
