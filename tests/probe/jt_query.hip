// jt_query.hip — TEST INFRASTRUCTURE ONLY: libjt_query.so, the product's traversal (csrc/jt_traverse.h)
// over arbitrary rays, one lane per ray, for tests/test_gpu_queries.py.
//
// The scene is laid out by the product's host code (csrc/jt_layout.cpp and jt_host.cpp are compiled
// into this library as the product Makefile's layout-check target compiles them), every array of
// JT_SCENE_ARRAYS is uploaded and the stack members of DScene are filled as upload_scene /
// alloc_stack_overflow (csrc/jt_trace.hip) fill them. A query kernel then runs, per lane, only
// functions of jt_traverse.h with COUNT = 1:
//     query_start<WIDE>; until query_done<WIDE>: prim_step if nprim > 0, else node_step_any;
//     then rerun_tie<WIDE>, and the loop again if it re-runs
// in one instantiation per traversal form the product builds (FORMS below). The LDS forms stage the
// blob and take blob_scene and bake_nodes from csrc/jt_kernels.h itself. Nothing here is linked
// into libjtrace_hip.so or covered by its source hash.
//
// Stack guard: every form's LDS stack holds what the form may use plus PUSH_SLOTS entries more, the
// overflow forms' HBM area `need` entries per lane plus PUSH_SLOTS; everything is filled with a
// canary before the query and a lane reports (flags) if an entry outside what it may use changed.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "jt_kernels.h"  // blob_scene, bake_nodes; jt_traverse.h through jt_integrator.h
#include "jt_layout.h"

using namespace jtd;
using namespace jtk;

namespace {

constexpr int CANARY = 0x5ca1ab1e;
constexpr int GUARD = PUSH_SLOTS;
constexpr int JQ_OUT = 16;       // ints per ray of jq_run's output
constexpr int JQ_STATE = 40;     // ints per query state of jq_run_leaf's output
constexpr int STEP_CAP = 1 << 22;  // steps of one lane's query before it gives up (flag 4)
enum { FLAG_LDS_GUARD = 1, FLAG_HBM_GUARD = 2, FLAG_STEP_CAP = 4, FLAG_OVER_BOUND = 8 };
constexpr size_t LDS_BLOB_BUDGET = 48 * 1024;  // the product's default lds_scene budget (jt_select.h)

// The traversal forms the product builds (CONFIGS, jt_select.h; trace_kernel / trace_kernel_lds):
// the feature masks the traversal can tell apart are those of FT_XFORM and FT_QUAD.
struct Form {
    const char* name;
    bool wide, ovf, lds;  // lds: the scene is the LDS blob (NCACHE false), else HBM pointers (NCACHE true)
    int feat;
};
constexpr int NFORMS = 15;
const Form FORMS[NFORMS] = {
    {"hbm_fixed/all", false, false, false, FT_ALL},                          // configuration 1, lds_scene=0
    {"hbm_fixed/none", false, false, false, FT_NONE | FT_LINL},              // 0 (and 7), lds_scene=0
    {"hbm_ovf/all", false, true, false, FT_ALL},                             // 5
    {"hbm_ovf/mesh", false, true, false, FT_MESH | FT_LINL},                 // 2
    {"hbm_ovf/mesh_env_quad", false, true, false, FT_MESH_ENV_QUAD | FT_LINL},  // 4
    {"lds_plan/all", false, false, true, FT_ALL},                            // 1: push_plan
    {"lds_baked/none", false, false, true, FT_NONE | FT_LINL},               // 0: bake_nodes + push_plan_baked
    {"lds_ovf/all", false, true, true, FT_ALL},                              // 5
    {"wide_hbm_fixed/all", true, false, false, FT_ALL},                      // 9
    {"wide_hbm_fixed/none", true, false, false, FT_NONE | FT_LINL},          // 8
    {"wide_hbm_ovf/all", true, true, false, FT_ALL},                         // 13
    {"wide_hbm_ovf/mesh", true, true, false, FT_MESH | FT_LINL},             // 10
    {"wide_hbm_ovf/mesh_env_quad", true, true, false, FT_MESH_ENV_QUAD | FT_LINL},  // 12
    {"wide_lds/all", true, false, true, FT_ALL},                             // 9
    {"wide_lds/none", true, false, true, FT_NONE | FT_LINL},                 // 8
};

struct Scene {
    jt::HostScene hs;
    DScene S{};
    std::vector<void*> allocs;
    std::vector<int> dev_to_ref;  // device instance id -> the reference's (hs.inst_new inverted)
    ~Scene() {
        for (void* p : allocs) (void)hipFree(p);
    }
};

template <class T>
hipError_t upload(Scene& sc, const std::vector<T>& host, const T** dptr) {
    const size_t bytes = host.empty() ? sizeof(T) : host.size() * sizeof(T);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    sc.allocs.push_back(p);
    if (!host.empty()) e = hipMemcpy(p, host.data(), bytes, hipMemcpyHostToDevice);
    *dptr = (const T*)p;
    return e;
}

__device__ __forceinline__ void fill_guarded_stack(int* stack, int entries) {
    for (int k = 0; k < entries; k++) stack[k * BLOCK] = CANARY;
}
__device__ __forceinline__ bool guard_changed(const int* stack, int from, int to, int stride) {
    bool bad = false;
    for (int k = from; k < to; k++) bad = bad || stack[(size_t)k * stride] != CANARY;
    return bad;
}

// One ray per lane. `entries`: the LDS stack entries per lane, guard included; `used`: how many of
// them the form may use (the scene's bound, or the ring entries in use); hbm_used: the entries of
// the lane's HBM overflow area it may use (the bound), GUARD more follow.
template <bool WIDE, bool OVF, bool LDS, int F>
__global__ __launch_bounds__(BLOCK) void jq_kernel(DScene S0, int n, const float* __restrict__ rays, const int* __restrict__ inst,
                                                  int* __restrict__ out, int entries, int used, int hbm_used) {
    constexpr bool NCACHE = !LDS;
    constexpr int RING = 16;
    constexpr int PB = push_bit(node_baked<OVF, NCACHE, WIDE, F>());
    extern __shared__ uint4 jq_lds[];
    int* const stack = reinterpret_cast<int*>(jq_lds) + threadIdx.x;
    fill_guarded_stack(stack, entries);
    DScene S = S0;
    if constexpr (LDS) {  // as trace_kernel_lds: the blob behind the stack, baked where the step wants it
        uint4* const blob = jq_lds + (size_t)entries * BLOCK * 4 / 16;
        for (int k = threadIdx.x; k < S0.blob_n16; k += BLOCK) blob[k] = S0.blob[k];
        __syncthreads();
        if constexpr (node_baked<OVF, NCACHE, WIDE, F>()) {
            bake_nodes(S0, blob);
            __syncthreads();
        }
        S = blob_scene(S0, blob);
    }
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const v3 o = V3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = V3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const int q = inst ? inst[i] : -1;
    Counters cnt{0, 0, 0, 0};
    Trav T;
    query_start<WIDE>(S, T, o, d, q, stack, 0, PB);
    int maxsp = T.sp, steps = 0, flags = 0;
    for (;;) {
        while (!query_done<WIDE>(T) && steps < STEP_CAP) {
            if (T.nprim > 0) prim_step<1, F>(S, T, cnt);
            else node_step_any<WIDE, RING, OVF, 1, NCACHE, F>(S, T, stack, i, cnt);
            maxsp = T.sp > maxsp ? T.sp : maxsp;
            steps++;
            // a stack above the scene's bound: stop before a later push could leave the guard
            // (the next step writes below sp + PUSH_SLOTS <= bound + 1 + GUARD - 1 after its pop)
            if (T.sp > hbm_used) steps = STEP_CAP + 1;
        }
        if (steps >= STEP_CAP) {
            flags |= steps > STEP_CAP ? FLAG_OVER_BOUND : FLAG_STEP_CAP;
            break;
        }
        if (!rerun_tie<WIDE>(S, T, o, d, q, stack, PB)) break;
    }
    if (guard_changed(stack, used, entries, BLOCK)) flags |= FLAG_LDS_GUARD;
    if (OVF && guard_changed(S.ovf + (size_t)i * S.ovf_stride, hbm_used, S.ovf_stride, 1)) flags |= FLAG_HBM_GUARD;
    const Hit h = query_hit(T);
    int* const y = out + (size_t)i * JQ_OUT;
    y[0] = h.inst;
    y[1] = h.elem;
    y[2] = __float_as_int(h.u);
    y[3] = __float_as_int(h.v);
    y[4] = __float_as_int(h.t);
    y[5] = h.hit ? 1 : 0;
    y[6] = T.nh & NH_COUNT;
    y[7] = (int)cnt.nodes;
    y[8] = (int)cnt.instances;
    y[9] = (int)cnt.prims;
    y[10] = maxsp;
    y[11] = flags;
    y[12] = T.nh;
    y[13] = steps;
    y[14] = 0;
    y[15] = 0;
}

// every field of a query's state and its counters, as 32-bit words
__device__ __forceinline__ void dump_state(const Trav& T, const Counters& c, int* y) {
    const v3* v[6] = {&T.wo, &T.wd, &T.wdinv, &T.lo, &T.ld, &T.ldinv};
    for (int k = 0; k < 6; k++) {
        y[3 * k] = __float_as_int(v[k]->x);
        y[3 * k + 1] = __float_as_int(v[k]->y);
        y[3 * k + 2] = __float_as_int(v[k]->z);
    }
    const int w[JQ_STATE - 18] = {__float_as_int(T.tmax), T.sp, T.low, T.inst_space, T.negmask, T.cur_inst, T.cur_kind, T.prim,
                                  T.nprim, T.h_inst, T.h_elem, __float_as_int(T.h_u), __float_as_int(T.h_v), T.nh, (int)T.nxt,
                                  (int)c.nodes, (int)c.instances, (int)c.prims, 0, 0, 0, 0};
    for (int k = 0; k < JQ_STATE - 18; k++) y[18 + k] = w[k];
}

// inst_leaf_query against what its comment promises: the state query_start + node_step leave, in the
// kernels that call it (LDS mode, binary, fixed stack). out: per ray the two states, JQ_STATE ints each.
template <int F>
__global__ __launch_bounds__(BLOCK) void jq_leaf_kernel(DScene S0, int n, const float* __restrict__ rays, const int* __restrict__ inst,
                                                       int* __restrict__ out, int entries) {
    constexpr int PB = push_bit(node_baked<false, false, false, F>());
    extern __shared__ uint4 jq_lds[];
    int* const stack = reinterpret_cast<int*>(jq_lds) + threadIdx.x;
    fill_guarded_stack(stack, entries);
    uint4* const blob = jq_lds + (size_t)entries * BLOCK * 4 / 16;
    for (int k = threadIdx.x; k < S0.blob_n16; k += BLOCK) blob[k] = S0.blob[k];
    __syncthreads();
    if constexpr (node_baked<false, false, false, F>()) {
        bake_nodes(S0, blob);
        __syncthreads();
    }
    const DScene S = blob_scene(S0, blob);
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const v3 o = V3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), d = V3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const int q = inst[i];
    Counters ca{0, 0, 0, 0}, cb{0, 0, 0, 0};
    Trav A, B;
    query_start<false>(S, A, o, d, q, stack, 0, PB);
    node_step<16, false, 1, false, F>(S, A, stack, i, ca);
    // dinv and negmask "are those of query_begin for direction d"
    const v3 dinv = V3(jl_rcp(d.x), jl_rcp(d.y), jl_rcp(d.z));
    inst_leaf_query<1, F>(S, B, o, d, dinv, neg_mask(d, S.order_flip | PB), q, cb);
    dump_state(A, ca, out + (size_t)i * 2 * JQ_STATE);
    dump_state(B, cb, out + (size_t)i * 2 * JQ_STATE + JQ_STATE);
}

// the smallest of FT_NONE, FT_MESH, FT_MESH_ENV_QUAD that covers the scene's features, else FT_ALL
int special_mask(int feat) {
    if (feat == FT_NONE) return FT_NONE;
    if (!(feat & ~FT_MESH)) return FT_MESH;
    if (!(feat & ~FT_MESH_ENV_QUAD)) return FT_MESH_ENV_QUAD;
    return FT_ALL;
}

template <bool WIDE, bool OVF, bool LDS, int F>
hipError_t launch(const DScene& S, int n, const float* rays, const int* inst, int* out, int entries, int used, int hbm_used,
                  size_t lds) {
    constexpr auto k = &jq_kernel<WIDE, OVF, LDS, F>;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), lds, 0, S, n, rays, inst, out, entries, used,
                       hbm_used);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int jq_form_count(void) { return NFORMS; }
const char* jq_form_name(int f) { return f >= 0 && f < NFORMS ? FORMS[f].name : nullptr; }
int jq_out_words(void) { return JQ_OUT; }
int jq_state_words(void) { return JQ_STATE; }

// Lays the scene out for params->traversal (0 reference, 1 near, 2 wide) and uploads it.
// Returns the layout's status (jt_last_error) or a HIP error as 1000 + code.
int jq_open(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params, void** out) {
    *out = nullptr;
    Scene* sc = new Scene();
    jt::HostScene& hs = sc->hs;
    int st = jt::layout_scene(scene, bvh, lights, params, jt::Options{}, hs);
    if (st != JT_OK) {
        delete sc;
        return st;
    }
    sc->dev_to_ref.assign(scene->ninstances, -1);
    for (int k = 0; k < scene->ninstances; k++) sc->dev_to_ref[hs.inst_new[k]] = k;
    DScene& S = sc->S;
    S = hs.S;
    hipError_t e = hipSuccess;
#define JQ_UPLOAD(T, name) \
    if (e == hipSuccess) e = upload(*sc, hs.name, &S.name);
    JT_SCENE_ARRAYS(JQ_UPLOAD, JQ_UPLOAD)
#undef JQ_UPLOAD
    if (e == hipSuccess) e = upload(*sc, hs.blob, &S.blob);
    S.blob_n16 = (int)hs.blob.size();
    S.ovf = nullptr;
    S.ovf_stride = 0;
    S.ring = 16;
    S.stack_need = hs.need;
    if (e != hipSuccess) {
        delete sc;
        return 1000 + (int)e;
    }
    *out = sc;
    return JT_OK;
}
void jq_close(void* h) { delete (Scene*)h; }
// The layout alone, no device: info = need, feat, blob bytes (a CPU test asserts a scene's bound with it).
int jq_layout_info(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                   int32_t* info) {
    jt::HostScene hs;
    const int st = jt::layout_scene(scene, bvh, lights, params, jt::Options{}, hs);
    if (st != JT_OK) return st;
    info[0] = hs.need;
    info[1] = hs.feat;
    info[2] = (int)(hs.blob.size() * 16);
    return JT_OK;
}
const char* jq_last_error(void) { return jt_last_error(); }

// info: need, feat, wide, order_flip, blob bytes, instances, the specialised mask
int jq_info(void* h, int32_t* info) {
    const Scene* sc = (const Scene*)h;
    info[0] = sc->hs.need;
    info[1] = sc->hs.feat;
    info[2] = sc->hs.wide ? 1 : 0;
    info[3] = sc->S.order_flip;
    info[4] = (int)(sc->hs.blob.size() * 16);
    info[5] = (int)sc->dev_to_ref.size();
    info[6] = special_mask(sc->hs.feat);
    return 0;
}
// per reference instance: 1 if its BLAS is one leaf (INST_LEAF_ROOT), else 0
int jq_leaf_roots(void* h, int32_t* out) {
    const Scene* sc = (const Scene*)h;
    for (size_t k = 0; k < sc->dev_to_ref.size(); k++) out[k] = (sc->hs.inst_blas[sc->hs.inst_new[k]].w & INST_LEAF_ROOT) ? 1 : 0;
    return 0;
}

// Why form f cannot run on this scene (a static string), or nullptr if it can.
const char* jq_form_skip(void* h, int f) {
    const Scene* sc = (const Scene*)h;
    if (f < 0 || f >= NFORMS) return "no such form";
    const Form& F = FORMS[f];
    const int feat = sc->hs.feat;
    if (F.wide != sc->hs.wide) return "the scene is laid out for the other record kind";
    if (feat & ~F.feat & FT_ALL) return "the mask does not cover the scene's features";
    if ((F.feat & FT_ALL) != FT_ALL && (F.feat & FT_ALL) != special_mask(feat)) return "not the smallest mask that covers the scene";
    if (!F.ovf && sc->hs.need > 16) return "stack bound above 16: the product runs the scene with overflow";
    if (F.lds && sc->hs.blob.size() * 16 > LDS_BLOB_BUDGET) return "blob above the LDS budget";
    return nullptr;
}

// n rays (o, d) through form f; inst: NULL, or per ray the reference's instance id (-1: scene
// query); ring: the entries of the LDS ring in use (overflow forms: 16 or 2). out: n x JQ_OUT ints:
// inst (reference numbering), elem, u, v, t bits, hit, nh & 63, nodes, instances, prims, the largest
// sp, flags (1 LDS guard changed, 2 HBM guard changed, 4 step cap, 8 sp above the bound), nh, steps.
// Returns 0, -1 for a form that cannot run (jq_form_skip) or bad arguments, 1000 + a HIP error,
// 2000 + the rays' flags or-ed together if any is set (a guard entry changed, ...).
int jq_run(void* h, int f, int ring, int64_t n, const float* rays, const int32_t* inst, int32_t* out) {
    Scene* sc = (Scene*)h;
    if (!sc || jq_form_skip(h, f) || n < 1 || n > (1 << 22)) return -1;
    const Form& F = FORMS[f];
    if (F.ovf ? (ring != 2 && ring != 16) : ring != 16) return -1;
    const int need = sc->hs.need, ninst = (int)sc->dev_to_ref.size();
    std::vector<int32_t> dinst;
    if (inst) {
        dinst.resize(n);
        for (int64_t i = 0; i < n; i++) {
            if (inst[i] >= ninst) return -1;
            dinst[i] = inst[i] < 0 ? -1 : sc->hs.inst_new[inst[i]];
            if (inst[i] >= 0 && dinst[i] < 0) return -1;
        }
    }
    // the LDS stack: the scene's bound (fixed) or the 16-entry ring, plus the guard
    const int used = F.ovf ? ring : need, entries = (F.ovf ? 16 : need) + GUARD;
    const size_t lds = (size_t)entries * BLOCK * 4 + (F.lds ? sc->hs.blob.size() * 16 : 0);
    if (lds > 160 * 1024) return -1;
    const size_t N = (size_t)n, lanes = (N + BLOCK - 1) / BLOCK * BLOCK;
    float* drays = nullptr;
    int *dins = nullptr, *dout = nullptr, *dovf = nullptr;
    DScene S = sc->S;
    S.ring = ring;
    hipError_t e = hipMalloc((void**)&drays, N * 6 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, N * JQ_OUT * sizeof(int));
    if (e == hipSuccess && inst) e = hipMalloc((void**)&dins, N * sizeof(int));
    if (e == hipSuccess && F.ovf) {
        S.ovf_stride = need + GUARD;
        e = hipMalloc((void**)&dovf, lanes * (size_t)S.ovf_stride * sizeof(int));
        if (e == hipSuccess) e = hipMemsetD32((hipDeviceptr_t)dovf, CANARY, lanes * (size_t)S.ovf_stride);
        S.ovf = dovf;
    }
    if (e == hipSuccess) e = hipMemcpy(drays, rays, N * 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && inst) e = hipMemcpy(dins, dinst.data(), N * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xff, N * JQ_OUT * sizeof(int));
    if (e == hipSuccess) {
#define JQ_CASE(ID, WIDE, OVF, LDS, FEAT) \
    case ID: e = launch<WIDE, OVF, LDS, FEAT>(S, (int)n, drays, dins, dout, entries, used, need, lds); break;
        switch (f) {
            JQ_CASE(0, false, false, false, FT_ALL)
            JQ_CASE(1, false, false, false, FT_NONE | FT_LINL)
            JQ_CASE(2, false, true, false, FT_ALL)
            JQ_CASE(3, false, true, false, FT_MESH | FT_LINL)
            JQ_CASE(4, false, true, false, FT_MESH_ENV_QUAD | FT_LINL)
            JQ_CASE(5, false, false, true, FT_ALL)
            JQ_CASE(6, false, false, true, FT_NONE | FT_LINL)
            JQ_CASE(7, false, true, true, FT_ALL)
            JQ_CASE(8, true, false, false, FT_ALL)
            JQ_CASE(9, true, false, false, FT_NONE | FT_LINL)
            JQ_CASE(10, true, true, false, FT_ALL)
            JQ_CASE(11, true, true, false, FT_MESH | FT_LINL)
            JQ_CASE(12, true, true, false, FT_MESH_ENV_QUAD | FT_LINL)
            JQ_CASE(13, true, false, true, FT_ALL)
            JQ_CASE(14, true, false, true, FT_NONE | FT_LINL)
        }
#undef JQ_CASE
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, N * JQ_OUT * sizeof(int), hipMemcpyDeviceToHost);
    int flags = 0;
    if (e == hipSuccess)
        for (size_t i = 0; i < N; i++) {
            int32_t& k = out[i * JQ_OUT];
            k = k >= 0 && k < ninst ? sc->dev_to_ref[k] : k;
            flags |= out[i * JQ_OUT + 11];
        }
    void* all[] = {drays, dins, dout, dovf};
    for (void* p : all)
        if (p) (void)hipFree(p);
    if (e != hipSuccess) return 1000 + (int)e;
    return flags ? 2000 + flags : 0;  // a changed canary, a runaway query or stack: an error (out is filled)
}

// inst_leaf_query and query_start + node_step on n rays, inst[i] a reference instance whose BLAS is
// one leaf (jq_leaf_roots), in the LDS fixed-stack binary form: baked 0 runs <FT_ALL>, 1 the baking
// <FT_NONE | FT_LINL> (matte identity-frame triangle scenes only). out: n x 2 x JQ_STATE ints,
// first the state node_step leaves, then inst_leaf_query's.
int jq_run_leaf(void* h, int baked, int64_t n, const float* rays, const int32_t* inst, int32_t* out) {
    Scene* sc = (Scene*)h;
    if (!sc || !inst || n < 1 || n > (1 << 22) || jq_form_skip(h, baked ? 6 : 5)) return -1;
    const int ninst = (int)sc->dev_to_ref.size();
    std::vector<int32_t> dinst(n);
    for (int64_t i = 0; i < n; i++) {
        if (inst[i] < 0 || inst[i] >= ninst) return -1;
        dinst[i] = sc->hs.inst_new[inst[i]];
        if (dinst[i] < 0 || !(sc->hs.inst_blas[dinst[i]].w & INST_LEAF_ROOT)) return -1;
    }
    const int entries = sc->hs.need + GUARD;
    const size_t lds = (size_t)entries * BLOCK * 4 + sc->hs.blob.size() * 16, N = (size_t)n;
    if (lds > 160 * 1024) return -1;
    float* drays = nullptr;
    int *dins = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&drays, N * 6 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, N * 2 * JQ_STATE * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&dins, N * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(drays, rays, N * 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dins, dinst.data(), N * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const void* k = baked ? (const void*)&jq_leaf_kernel<FT_NONE | FT_LINL> : (const void*)&jq_leaf_kernel<FT_ALL>;
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        const dim3 grid((unsigned)((N + BLOCK - 1) / BLOCK)), block(BLOCK);
        if (e == hipSuccess) {
            if (baked) hipLaunchKernelGGL(jq_leaf_kernel<FT_NONE | FT_LINL>, grid, block, lds, 0, sc->S, (int)n, drays, dins, dout, entries);
            else hipLaunchKernelGGL(jq_leaf_kernel<FT_ALL>, grid, block, lds, 0, sc->S, (int)n, drays, dins, dout, entries);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, N * 2 * JQ_STATE * sizeof(int), hipMemcpyDeviceToHost);
    void* all[] = {drays, dins, dout};
    for (void* p : all)
        if (p) (void)hipFree(p);
    return e == hipSuccess ? 0 : 1000 + (int)e;
}

}  // extern "C"
