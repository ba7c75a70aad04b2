// Slot plan of the chunked oscillator (ddsp_osc_chunk.hip): which harmonic each of a lane's K register slots holds.
// Plain C++ (no HIP), so that a host test can compile it on its own.
//
// The unwrapped fp32 phase of harmonic 2^t * r is bit for bit 2^t times the phase of harmonic r (every rounding on the way
// commutes with a power of two: DESIGN.md §4a), so only some slots -- ROOTS -- walk the increment / fp64 accumulate chain;
// a DERIVED slot takes the rounded phase of a root slot of the same lane times 2^t.  Registers cannot be indexed per
// lane, so WHICH root a derived slot reads, and with which t, is fixed at compile time per K (slot_children below: root slot i
// feeds slot_children(K, i) derived slots, the r-th of them with t = r + 1: derived_shift); the planner's job is to cut the odd families o, 2o, 4o, ... into pieces
// {r, r * 2^t1, r * 2^t2, ...} that fill G lanes of that one shape.  Where it cannot, the launch keeps the all-roots
// mapping (harmonic = lane + slot * G).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <set>
#include <type_traits>
#include <vector>

namespace ddsp_osc {

constexpr int kPlanMaxLanes = 16, kPlanMaxK = 25, kPlanMaxSlots = kPlanMaxLanes * kPlanMaxK;
constexpr int kPlanParents = 7;         // root slots that may feed derived ones
constexpr int kPlanMaxChildren = 3;     // derived slots per root slot
constexpr uint16_t kNoHarmonic = 0xffff;

// THE list of K -- harmonics per lane, a template parameter of every oscillator kernel -- with, per K, the derived slots fed by
// root slots 0..6.  Everything that enumerates K derives from it: kOscKs, dispatch_k, slot_children.  The children are
// non-increasing in the root slot: small harmonics have the long families.  Found by exhaustive search over the shapes with the
// most derived slots that pack every (H, K, G) the tilings select (tests/test_osc_slot_plan_host.py).
#define DDSP_OSC_KS(X)                                                                                                  \
    X(4, 1, 0, 0, 0, 0, 0, 0) X(8, 2, 1, 0, 0, 0, 0, 0) X(12, 3, 2, 1, 0, 0, 0, 0) X(13, 3, 2, 1, 0, 0, 0, 0)         \
    X(15, 3, 2, 1, 1, 0, 0, 0) X(16, 3, 2, 1, 1, 0, 0, 0) X(20, 3, 2, 2, 1, 1, 0, 0) X(23, 3, 2, 2, 1, 1, 1, 0)       \
    X(25, 3, 2, 2, 1, 1, 1, 1)

#define DDSP_K_VALUE(KK, ...) KK,
constexpr int kOscKs[] = {DDSP_OSC_KS(DDSP_K_VALUE)};
#undef DDSP_K_VALUE

// f(std::integral_constant<int, K>{}) for a listed K, `unknown` for any other
template <class F, class R>
R dispatch_k(int K, F &&f, R unknown)
{
    switch (K) {
#define DDSP_K_CASE(KK, ...) case KK: return f(std::integral_constant<int, KK>{});
        DDSP_OSC_KS(DDSP_K_CASE)
#undef DDSP_K_CASE
        default: return unknown;
    }
}

constexpr int pick7(int i, int a, int b, int c, int d, int e, int f, int g)
{
    return i == 0 ? a : i == 1 ? b : i == 2 ? c : i == 3 ? d : i == 4 ? e : i == 5 ? f : i == 6 ? g : 0;
}
// Derived slots fed by root slot i.
constexpr int slot_children(int K, int i)
{
    switch (K) {
#define DDSP_K_CHILDREN(KK, ...) case KK: return pick7(i, __VA_ARGS__);
        DDSP_OSC_KS(DDSP_K_CHILDREN)
#undef DDSP_K_CHILDREN
        default: return 0;
    }
}
constexpr bool plan_covers_every_k()
{
    for (int K : kOscKs)
        if (K > kPlanMaxK || slot_children(K, 0) < 1) return false;
    return true;
}
static_assert(plan_covers_every_k(), "every listed K needs a slot_children shape and kPlanMaxK must bound it");
constexpr int plan_derived(int K)
{
    int n = 0;
    for (int i = 0; i < kPlanParents; ++i) n += slot_children(K, i);
    return n;
}
constexpr int plan_roots(int K) { return K - plan_derived(K); }
// Derived slots are numbered root slot by root slot (all children of root slot 0, then of root slot 1, ...): derived slot d is
// child number derived_rank(K, d) of root slot derived_parent(K, d), and the children of the first n root slots are a prefix.
constexpr int derived_parent(int K, int d)
{
    int n = 0;
    for (int i = 0; i < kPlanParents; ++i)
        for (int r = 0; r < slot_children(K, i); ++r) {
            if (n == d) return i;
            ++n;
        }
    return 0;
}
constexpr int derived_rank(int K, int d)
{
    int n = 0;
    for (int i = 0; i < kPlanParents; ++i)
        for (int r = 0; r < slot_children(K, i); ++r) {
            if (n == d) return r;
            ++n;
        }
    return 0;
}
// A FILLED derived slot d holds 2^t times its root's harmonic number with t = derived_shift(K, d): plan_slots cuts every odd
// family into contiguous runs {r, 2r, 4r, ...} and gives child number c of a run to the root slot's child of rank c, so t is a
// property of the slot, the same in every lane (tests/test_osc_plan_shift_host.py holds this for every K, G and H = 1..400).  The
// kernels take the factor from here, at compile time; PlanTable::shift records the same t per lane (0 in a padded slot).
constexpr int derived_shift(int K, int d) { return derived_rank(K, d) + 1; }
// Silent-harmonic classes: class q = 0..3 walks the first class_prefix(KR, q) root slots (3/4, 1/2, 1/4, 1/8 of them) and the
// derived slots they feed, class_derived(K, that many); a wavefront whose highest audible harmonic number is <= cls_max[q]
// may take it.
constexpr int class_prefix(int n, int q) { return q == 0 ? (3 * n + 3) / 4 : q == 1 ? (n + 1) / 2 : q == 2 ? (n + 3) / 4 : (n + 7) / 8; }
constexpr int class_derived(int K, int nroots)
{
    int n = 0;
    for (int i = 0; i < kPlanParents && i < nroots; ++i) n += slot_children(K, i);
    return n;
}

// What the kernels read (by value in the kernel arguments): [lane * K + slot], root slots first.
struct PlanTable {
    uint16_t h[kPlanMaxSlots];      // 0-based harmonic of the slot, kNoHarmonic = padding (amplitude 0)
    uint8_t shift[kPlanMaxSlots];   // derived slots: t, the slot's phase is its root's times 2^t
};

struct SlotPlan {
    int H, K, G;
    int KR, KD;          // root and derived slots per lane (KD = 0: all-roots mapping)
    int cls_max[4];      // highest audible harmonic NUMBER (1-based, 0 = silent) that class q's prefixes still hold
    PlanTable t;
};

inline void plan_class_limits(SlotPlan &pl)
{
    for (int q = 0; q < 4; ++q) {
        const int nr = class_prefix(pl.KR, q), nd = pl.KD ? class_derived(pl.K, nr) : 0;
        int lim = pl.H;
        for (int j = 0; j < pl.G; ++j)
            for (int m = 0; m < pl.K; ++m) {
                const bool inside = m < pl.KR ? m < nr : m - pl.KR < nd;
                const int h = pl.t.h[j * pl.K + m];
                if (!inside && h != kNoHarmonic) lim = std::min(lim, h);   // harmonic number h + 1 is outside: h is the limit
            }
        pl.cls_max[q] = lim;
    }
}

// today's mapping: every slot a root, harmonic = lane + slot * G
inline void plan_all_roots(int H, int K, int G, SlotPlan &pl)
{
    pl.H = H; pl.K = K; pl.G = G; pl.KR = K; pl.KD = 0;
    for (int i = 0; i < kPlanMaxSlots; ++i) { pl.t.h[i] = kNoHarmonic; pl.t.shift[i] = 0; }
    for (int j = 0; j < G; ++j)
        for (int m = 0; m < K; ++m)
            if (j + m * G < H) pl.t.h[j * K + m] = (uint16_t)(j + m * G);
    plan_class_limits(pl);
}

namespace plan_detail {
struct Piece { int size_class; std::vector<int> members; };   // members[0] = root (harmonic numbers, 1-based)
struct Search {
    std::vector<std::vector<int>> chains;   // odd families, longest first
    int cnt[kPlanMaxChildren + 2];          // free root slots by piece size 1..4 (over all lanes)
    std::vector<Piece> pieces;
    std::set<std::vector<int>> dead;        // (chain, cnt[]) states that cannot be completed

    // cut chain ci from element `at` on into pieces no longer than `maxp` (non-increasing), each into the smallest free size class
    bool cut(int ci, int at, int maxp)
    {
        const std::vector<int> &ch = chains[ci];
        const int left = (int)ch.size() - at;
        if (left == 0) return place(ci + 1);
        for (int p = std::min(left, maxp); p >= 1; --p) {
            int s = p;
            while (s <= kPlanMaxChildren + 1 && cnt[s] == 0) ++s;
            if (s > kPlanMaxChildren + 1) continue;
            --cnt[s];
            pieces.push_back(Piece{s, std::vector<int>(ch.begin() + at, ch.begin() + at + p)});
            if (cut(ci, at + p, p)) return true;
            pieces.pop_back();
            ++cnt[s];
        }
        return false;
    }
    bool place(int ci)
    {
        if (ci == (int)chains.size()) return true;
        std::vector<int> key = {ci, cnt[1], cnt[2], cnt[3], cnt[4]};
        if (dead.count(key)) return false;
        if (cut(ci, 0, kPlanMaxChildren + 1)) return true;
        dead.insert(key);
        return false;
    }
};
}  // namespace plan_detail

// The plan with derived slots for (H, K, G), or false where the shape of K cannot be packed (callers then use plan_all_roots).
// The chunk totals keep one column per root slot, KR * G of them, where the all-roots form keeps H: a plan is only taken
// when that is no more (the scratch buffer is sized by H).
inline bool plan_slots(int H, int K, int G, SlotPlan &pl)
{
    using namespace plan_detail;
    const int KD = plan_derived(K), KR = K - KD;
    if (KD < 1 || H < 1 || G < 1 || G > kPlanMaxLanes || K > kPlanMaxK || G * K < H || KR * G > H) return false;
    Search s;
    for (int o = 1; o <= H; o += 2) {
        std::vector<int> ch;
        for (int x = o; x <= H; x *= 2) ch.push_back(x);
        s.chains.push_back(ch);
    }
    std::stable_sort(s.chains.begin(), s.chains.end(),
                     [](const std::vector<int> &a, const std::vector<int> &b) { return a.size() > b.size(); });
    for (int i = 0; i <= kPlanMaxChildren + 1; ++i) s.cnt[i] = 0;
    for (int i = 0; i < KR; ++i) s.cnt[1 + slot_children(K, i)] += G;
    if (!s.place(0)) return false;

    pl.H = H; pl.K = K; pl.G = G; pl.KR = KR; pl.KD = KD;
    for (int i = 0; i < kPlanMaxSlots; ++i) { pl.t.h[i] = kNoHarmonic; pl.t.shift[i] = 0; }
    // per size class: pieces by ascending root, dealt to the root slots of that size slot by slot (one per lane), so that a
    // slot index holds harmonics of similar height in every lane
    int derived = 0;
    for (int sz = kPlanMaxChildren + 1; sz >= 1; --sz) {
        std::vector<const Piece *> ps;
        for (const Piece &p : s.pieces)
            if (p.size_class == sz) ps.push_back(&p);
        std::sort(ps.begin(), ps.end(), [](const Piece *a, const Piece *b) { return a->members[0] < b->members[0]; });
        std::vector<int> idx;
        for (int i = 0; i < KR; ++i)
            if (1 + slot_children(K, i) == sz) idx.push_back(i);
        for (size_t n = 0; n < ps.size(); ++n) {
            const int i = idx[n / G], j = (int)(n % G);
            const std::vector<int> &mem = ps[n]->members;
            pl.t.h[j * K + i] = (uint16_t)(mem[0] - 1);
            for (size_t c = 1; c < mem.size(); ++c) {
                int d = 0;
                while (!(derived_parent(K, d) == i && derived_rank(K, d) == (int)c - 1)) ++d;
                int t = 0;
                while ((mem[0] << t) < mem[c]) ++t;
                pl.t.h[j * K + KR + d] = (uint16_t)(mem[c] - 1);
                pl.t.shift[j * K + KR + d] = (uint8_t)t;
                ++derived;
            }
        }
    }
    if (derived < 1) return false;
    plan_class_limits(pl);
    return true;
}

}  // namespace ddsp_osc
