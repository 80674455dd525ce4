// Traversal order of a scene's ray samples in the inference render launches of k_chain, written ONCE for both sides (as
// gnr_pack_body.h is for the packer): the device sort (k_sample_order, gnr_kernels.hip) and its host twin (gnr_sample_order_host,
// gnr_capi.inc) place sample i with the same two functions, so the two permutations are equal entry for entry.
//
// key of a sample = one byte, bit v set iff the sample projects inside view v (project_view's m != 0).  k_chain skips a view for a
// 16-sample tile only when all 16 samples are outside it, so samples are grouped by key:
//   1. stable counting sort by key; the groups in the order of key_before(): more views first (the long tiles lead, the launch's
//      tail is made of short ones), equal popcounts by descending key value;
//   2. the sorted sequence is cut into 16-sample groups and the groups are dealt round-robin into STRIPES stripes of the scene's
//      tile range (k_chain hands every XCD a contiguous eighth of the launch's tile list: without the stripes a launch of fewer
//      than 8 scenes would give one XCD all the full-length tiles).
// A scene's last tile holds P - 16 (tps - 1) samples; the sorted group that is dealt to it is the short one, wherever it sits in the
// sorted sequence, so that slot_of() is a bijection of [0, P) for every P.
// Results of k_chain do not depend on the order (a point's outputs do not depend on its tile): a wrong key or a wrong order can only
// cost speed.
#pragma once

#if defined(__HIPCC__)
#define GNR_SO_HD __host__ __device__
#else
#define GNR_SO_HD
#endif

namespace gnr {
namespace sorder {

constexpr int STRIPES = 8;
constexpr int TILE = 16;

GNR_SO_HD constexpr int popcount8(int k) { k = (k & 0x55) + ((k >> 1) & 0x55); k = (k & 0x33) + ((k >> 2) & 0x33); return (k & 0x0f) + (k >> 4); }

// does the group of key a come before the group of key b?
GNR_SO_HD constexpr bool key_before(int a, int b) {
    const int pa = popcount8(a), pb = popcount8(b);
    return pa != pb ? pa > pb : a > b;
}

// ---- the placement by chunks (k_sample_order and its serial host twin gnr_sample_order_host_chunked) ----
// A scene's samples are cut into chunks of `chunk` consecutive samples, and a chunk places its samples from the keys alone:
//   hist[k]    samples of key k in the scene,                      before[k]  those of them in front of the chunk,
//   by_rank[r] = hist[key of rank r], rank = key_rank() = the key's place in the key_before() order,
//   scan[r]    = by_rank[0] + .. + by_rank[r - 1] = start of the group of that key in the sorted sequence.
// Sample i of key k with `rank_in_chunk` samples of key k in front of it inside its chunk stands at chunk_pos() of the sorted sequence
// (= start[k] + #{ j < i : key_j == k }, what gnr_sample_order_host counts one sample after the other), and in slot slot_of() of it.
constexpr int KEYS = 256;
struct KeyRanks { unsigned char r[KEYS]; };
constexpr KeyRanks make_key_ranks() {
    KeyRanks t{};
    for (int k = 0; k < KEYS; ++k) {
        int n = 0;
        for (int k2 = 0; k2 < KEYS; ++k2) n += key_before(k2, k) ? 1 : 0;
        t.r[k] = (unsigned char)n;
    }
    return t;
}
// number of keys whose group comes before the group of key k (a bijection of 0..255: key_before is a strict total order)
GNR_SO_HD inline int key_rank(int k) {
    constexpr KeyRanks t = make_key_ranks();
    return t.r[k];
}
GNR_SO_HD inline int chunk_pos(const int* scan, const int* before, int k, int rank_in_chunk) { return scan[key_rank(k)] + before[k] + rank_in_chunk; }

// tiles of stripe s of a scene with tps tiles: the sorted groups s, s + STRIPES, s + 2 STRIPES, ...
GNR_SO_HD inline int stripe_tiles(int tps, int s) { return (tps - s + STRIPES - 1) / STRIPES; }

// position `pos` of the key-sorted sequence of a scene's P samples -> slot of the scene's (tile, row) list
GNR_SO_HD inline int slot_of(int pos, int P) {
    const int tps = (P + TILE - 1) / TILE;
    const int rem = P - (tps - 1) * TILE;                                     // samples of the last tile, 1..16
    const int gshort = tps <= STRIPES ? tps - 1 : STRIPES * (tps / STRIPES) - 1;   // sorted group that is dealt to the last tile
    int gi, wi;
    if (pos < TILE * gshort) { gi = pos / TILE; wi = pos % TILE; }
    else if (pos < TILE * gshort + rem) { gi = gshort; wi = pos - TILE * gshort; }
    else { const int q = pos + TILE - rem; gi = q / TILE; wi = q % TILE; }
    const int s = gi % STRIPES;
    int tile = gi / STRIPES;
    for (int k = 0; k < s; ++k) tile += stripe_tiles(tps, k);
    return tile * TILE + wi;
}

}  // namespace sorder
}  // namespace gnr
