// jt_multihit.h — the rules of the multi-hit queries (include/jtrace.h: jt_intersect_multi,
// jt_count_hits; the kernel and the context's half are in jt_multihit.hip) that need
// no device: the key that orders a ray's hits, the insertion into its sorted list of at most k
// records, the query's tmax after an insertion, the argument rule of k and the host variant's chunks.
// Plain C++ (no HIP runtime), shared by the kernel and the host check (tests/multihit_check.cpp).
// Not part of the ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "jt_intersect.h"  // QUERY_MAX_RAYS

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JT_MULTI_HD __host__ __device__ inline
#else
#define JT_MULTI_HD inline
#endif

namespace jtm {

constexpr int MULTI_MAX_HITS = 16;                        // JT_MULTI_MAX_HITS: the most records per ray
constexpr int64_t MULTI_MAX_RECORDS = (int64_t)1 << 30;   // n * k of one call, at most
constexpr int64_t MULTI_CHUNK_RECORDS = (int64_t)1 << 22;  // records of one chunk of the host variant, at most

// A list entry: jt_hit's six words, the instance in the caller's numbering.
struct MultiRec {
    int32_t inst, elem;
    float u, v, t;
    int32_t hit;
};
constexpr MultiRec multi_miss() { return MultiRec{-1, -1, 0.0f, 0.0f, __builtin_inff(), 0}; }

// The order of a ray's hits: (t, instance, element) ascending, t compared as float32. A NaN t is
// smaller than nothing and nothing is smaller than it.
JT_MULTI_HD bool multi_key_less(float t, int32_t inst, int32_t elem, float t2, int32_t inst2, int32_t elem2) {
    return t < t2 || (t == t2 && (inst < inst2 || (inst == inst2 && elem < elem2)));
}
JT_MULTI_HD bool multi_key_less(const MultiRec& a, const MultiRec& b) { return multi_key_less(a.t, a.inst, a.elem, b.t, b.inst, b.elem); }

// Candidate r meets a sorted list of `count` <= k entries (L.load(j), L.store(j, rec); entry j of
// the ray's own records). It goes in front of every trailing entry it is smaller than, found from the
// end; those move up one slot and, from a full list, the last one is dropped. Returns r's position,
// or k: a full list whose last entry is not larger, nothing written. *last: the t of entry k - 1
// afterwards, where an insertion leaves the list full.
// At most k loads and k stores; no entry outside [0, k) is touched.
template <class List>
JT_MULTI_HD int multi_insert(List& L, int k, int count, const MultiRec& r, float* last) {
    int j = count;
    float tl = r.t;
    while (j > 0) {
        const MultiRec e = L.load(j - 1);
        if (!multi_key_less(r, e)) break;
        if (j < k) {
            L.store(j, e);
            if (j == k - 1) tl = e.t;
        }
        j--;
    }
    if (j < k) L.store(j, r);
    *last = tl;
    return j;
}
// the list's length after multi_insert returned pos
JT_MULTI_HD int multi_count_after(int k, int count, int pos) { return pos < k && count < k ? count + 1 : count; }
// The query's tmax after multi_insert returned pos and *last: the caller's bound while the list holds
// fewer than k entries, the k-th entry's t once it is full; unchanged where nothing was inserted.
JT_MULTI_HD float multi_tmax_after(int k, int count_after, int pos, float last, float tmax) {
    return pos < k && count_after == k ? last : tmax;
}

// k of a call of n rays (n already within 0 .. QUERY_MAX_RAYS): the message, else nullptr
constexpr const char* multi_k_error(int64_t n, int32_t k) {
    return k < 1                                 ? "k must be at least 1"
           : k > MULTI_MAX_HITS                  ? "k must be at most JT_MULTI_MAX_HITS (16)"
           : n * (int64_t)k > MULTI_MAX_RECORDS  ? "k: n * k must be at most 2^30 records"
                                                 : nullptr;
}

// Rays of one chunk of jt_intersect_multi's host variant: n x k records do not fit the ray queries'
// 24-byte result slot per ray, so the array runs in chunks of at most floor(2^22 / k) rays through a
// buffer of the call's own. The option test_multi_chunk (tests only) lowers it.
constexpr int64_t multi_chunk(int32_t k, int64_t option) {
    const int64_t most = MULTI_CHUNK_RECORDS / (k < 1 ? 1 : k);
    return option >= 1 && option < most ? option : most;
}

}  // namespace jtm
