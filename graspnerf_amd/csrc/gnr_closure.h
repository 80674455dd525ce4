// What the graph operators over the parts share (gnr_support.hip: carried, grounded; gnr_balance.hip: what falls with a part that tips):
// the closure of a 256-bit set under a relation kept in LDS as one 256-bit row per part, run by one thread with the set in registers
// (every word index is a compile-time constant: no scratch).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace gnr {

constexpr int CLOSURE_PARTS = 256, CLOSURE_WORDS = CLOSURE_PARTS / 32;         // GNR_SUPPORT_MAX_PARTS, GNR_BALANCE_MAX_PARTS

// S |= everything reachable from the parts of `todo` along `rows` (S holds `todo` already).  A sweep takes the words of the work list
// in turn and expands every part of a word, those that join it meanwhile too; a part is expanded once in all, so a word gives at most
// 32 expansions per sweep, and a sweep that finds work expands at least one part: at most CLOSURE_PARTS sweeps.  stop: (when not null)
// end as soon as S meets it.  -> whether S meets `stop`.
__device__ inline bool close_over(const unsigned (*rows)[CLOSURE_WORDS], unsigned (&S)[CLOSURE_WORDS], unsigned (&todo)[CLOSURE_WORDS],
                                  const unsigned* stop) {
    for (int sweep = 0; sweep <= CLOSURE_PARTS; ++sweep) {
        bool any = false, met = false;
#pragma unroll
        for (int w = 0; w < CLOSURE_WORDS; ++w) {
            any = any || todo[w] != 0u;
            if (stop) met = met || (S[w] & stop[w]) != 0u;
        }
        if (met) return true;
        if (!any) return false;
#pragma unroll
        for (int w = 0; w < CLOSURE_WORDS; ++w) {
            for (int q = 0; q < 32 && todo[w]; ++q) {
                const int c = w * 32 + __ffs((int)todo[w]) - 1;
                todo[w] &= todo[w] - 1u;
#pragma unroll
                for (int v = 0; v < CLOSURE_WORDS; ++v) {
                    const unsigned fresh = rows[c][v] & ~S[v];
                    S[v] |= fresh;
                    todo[v] |= fresh;
                }
            }
        }
    }
    return false;
}

__device__ inline int bits_of(const unsigned (&S)[CLOSURE_WORDS]) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < CLOSURE_WORDS; ++w) c += __popc(S[w]);
    return c;
}

}  // namespace gnr
