// multihit_check.cpp — the rules of the multi-hit queries' list (csrc/jt_multihit.h) enumerated on the
// host. tests/test_multihit_host.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
//   - multi_key_less is a strict order on (t, instance, element), t first;
//   - multi_insert, for k = 1 .. 4 and every sequence of up to six candidates over a small key
//     space (equal-t pairs and triples among them): after every step the list is the k smallest
//     keys seen so far, ascending, the returned position is where the candidate stands (k: it was
//     refused), no slot outside [0, k) is touched, and tmax is the bound until the list is full
//     and the last entry's t from then on;
//   - eviction: a full list drops exactly its last entry, and a candidate equal to it in t is
//     decided by the ids;
//   - multi_k_error and multi_chunk at their boundaries.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_multihit.h"

namespace {

long cases = 0, bad = 0;
void check(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "multihit_check: %s (%lld %lld %lld)\n", what, a, b, c);
}

using jtm::MultiRec;

// a list of exactly k slots on the heap: the sanitizer sees any access outside it
struct HostList {
    std::vector<MultiRec> rec;
    int loads = 0, stores = 0;
    explicit HostList(int k) : rec((size_t)k, jtm::multi_miss()) {}
    MultiRec load(int j) {
        loads++;
        return rec.at((size_t)j);
    }
    void store(int j, const MultiRec& r) {
        stores++;
        rec.at((size_t)j) = r;
    }
};

bool same(const MultiRec& a, const MultiRec& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check_key() {
    const float ts[] = {0.5f, 1.0f, 2.0f};
    std::vector<MultiRec> keys;
    for (float t : ts)
        for (int i = 0; i < 3; i++)
            for (int e = 0; e < 3; e++) keys.push_back(MultiRec{i, e, 0, 0, t, 1});
    for (size_t a = 0; a < keys.size(); a++)
        for (size_t b = 0; b < keys.size(); b++) {
            // the enumeration order above is the key order
            check(jtm::multi_key_less(keys[a], keys[b]) == (a < b), "the key order", (long long)a, (long long)b);
            check(!(jtm::multi_key_less(keys[a], keys[b]) && jtm::multi_key_less(keys[b], keys[a])), "asymmetry");
        }
    const float nan = __builtin_nanf("");
    check(!jtm::multi_key_less(nan, 0, 0, 1.0f, 0, 0) && !jtm::multi_key_less(1.0f, 0, 0, nan, 0, 0), "a NaN t is smaller than nothing");
}

// every sequence of `len` candidates out of `pool`, inserted into a list of k
void check_sequences(int k, const std::vector<MultiRec>& pool, int len) {
    const float bound = 100.0f;
    std::vector<int> pick((size_t)len, 0);
    for (;;) {
        HostList L(k);
        std::vector<MultiRec> seen;
        int count = 0;
        float tmax = bound;
        for (int s = 0; s < len; s++) {
            MultiRec r = pool[(size_t)pick[(size_t)s]];
            r.u = (float)s;  // tells candidates of one key apart
            if (!(r.t <= tmax)) continue;  // the primitive test refuses it at the current tmax
            float last = -1;
            L.loads = L.stores = 0;
            const int pos = jtm::multi_insert(L, k, count, r, &last);
            check(L.loads <= k && L.stores <= k, "at most k loads and k stores", k, L.loads, L.stores);
            const int after = jtm::multi_count_after(k, count, pos);
            tmax = jtm::multi_tmax_after(k, after, pos, last, tmax);
            count = after;
            // the model: a stable sort of everything seen keeps earlier candidates of one key in front
            seen.insert(std::upper_bound(seen.begin(), seen.end(), r, [](const MultiRec& a, const MultiRec& b) { return jtm::multi_key_less(a, b); }), r);
            const int want = (int)std::min(seen.size(), (size_t)k);
            check(count == want, "the count", k, count, want);
            bool ok = true;
            for (int j = 0; j < want; j++) ok = ok && same(L.rec[(size_t)j], seen[(size_t)j]);
            check(ok, "the list is the k smallest keys so far, ascending", k, s);
            for (int j = want; j < k; j++) check(same(L.rec[(size_t)j], jtm::multi_miss()), "a slot past the count was written", k, j);
            if (pos < k) check(same(L.rec[(size_t)pos], r), "the returned position holds the candidate", k, pos);
            else check(count == k && !jtm::multi_key_less(r, L.rec[(size_t)k - 1]), "a refused candidate is not smaller than the last entry", k);
            check(tmax == (count == k ? L.rec[(size_t)k - 1].t : bound), "tmax: the bound, then the k-th entry's t", k, count);
            if ((int)seen.size() > k) seen.resize((size_t)k);  // what was dropped never returns
        }
        int d = 0;
        while (d < len && ++pick[(size_t)d] == (int)pool.size()) pick[(size_t)d++] = 0;
        if (d == len) break;
    }
}

void check_insert() {
    // three distances, an equal-t pair and an equal-t triple among the keys
    const std::vector<MultiRec> pool = {
        {0, 0, 0, 0, 1.0f, 1}, {0, 1, 0, 0, 1.0f, 1}, {1, 0, 0, 0, 1.0f, 1}, {0, 2, 0, 0, 2.0f, 1},
        {2, 0, 0, 0, 2.0f, 1}, {1, 5, 0, 0, 3.0f, 1}, {0, 7, 0, 0, 0.5f, 1},
    };
    for (int k = 1; k <= 4; k++)
        for (int len = 1; len <= 5; len++) check_sequences(k, pool, len);
    // eviction at an equal t: the ids decide, whatever the arrival order
    for (int first = 0; first < 2; first++) {
        HostList L(1);
        float last, tmax = 9;
        const MultiRec a{3, 4, 0, 0, 1.5f, 1}, b{3, 2, 0, 0, 1.5f, 1};
        int count = 0;
        for (const MultiRec& r : {first ? a : b, first ? b : a}) {
            const int pos = jtm::multi_insert(L, 1, count, r, &last);
            count = jtm::multi_count_after(1, count, pos);
            tmax = jtm::multi_tmax_after(1, count, pos, last, tmax);
        }
        check(same(L.rec[0], b) && count == 1 && tmax == 1.5f, "k = 1 keeps the smallest id of an exact-t tie", first);
    }
}

void check_rules() {
    auto has = [](const char* msg, const char* word) { return msg && std::strstr(msg, word) != nullptr; };
    const int64_t M = jtq::QUERY_MAX_RAYS;
    check(jtm::multi_k_error(0, 1) == nullptr && jtm::multi_k_error(M, 1) == nullptr, "k = 1 fits every n");
    check(jtm::multi_k_error(M / 16, 16) == nullptr, "n * k = 2^30 is in range");
    check(has(jtm::multi_k_error(M / 16 + 1, 16), "k"), "n * k = 2^30 + 16");
    check(has(jtm::multi_k_error(M / 2 + 1, 2), "n * k"), "n * k just past 2^30");
    check(has(jtm::multi_k_error(1, 0), "k must be at least 1") && has(jtm::multi_k_error(1, -5), "k must"), "k < 1");
    check(has(jtm::multi_k_error(0, 17), "k must be at most") && jtm::multi_k_error(0, 16) == nullptr, "k > JT_MULTI_MAX_HITS");
    check(has(jtm::multi_k_error(1, INT32_MAX), "k must be at most"), "a huge k does not wrap");
    for (int k = 1; k <= jtm::MULTI_MAX_HITS; k++) {
        const int64_t c = jtm::multi_chunk(k, 0);
        check(c == ((int64_t)1 << 22) / k && c * k <= ((int64_t)1 << 22) && (c + 1) * k > ((int64_t)1 << 22), "floor(2^22 / k) rays", k, c);
        check(jtm::multi_chunk(k, -3) == c && jtm::multi_chunk(k, c) == c && jtm::multi_chunk(k, c + 1) == c, "an option that lowers nothing", k);
        check(jtm::multi_chunk(k, 1) == 1 && jtm::multi_chunk(k, c - 1) == c - 1 && jtm::multi_chunk(k, 1500) == 1500, "the option lowers the chunk", k);
    }
}

}  // namespace

int main() {
    check_key();
    check_insert();
    check_rules();
    std::printf("multihit_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
