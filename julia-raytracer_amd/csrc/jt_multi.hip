// jt_multi.hip — the multi-device context (include/jtrace.h jt_create_multi): one sub-context per
// device, each tracing its share of every batch into its own running mean, and the RCCL reduce
// of those means onto device 0 when they are read. The ABI functions (jt_trace.hip, jt_denoise.hip)
// hand a multi-device context to the multi_* functions here (jt_context.h).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "jt_context.h"
#include "jt_denoise.h"

// The multi-device state of a context: one sub-context per device; RCCL communicators for the
// reduce of jt_get_image
struct jtc::MultiCtx {
    std::vector<jt_ctx*> sub;
    std::vector<ncclComm_t> comms;
    std::vector<long long> nsub;  // samples accumulated by each device
    // split of every batch: false = contiguous sample shares (device d's mean weighted n_d / N in
    // the reduce), true = interleaved 8x8 pixel tiles (tile t on device t mod D, every sample of
    // the batch; disjoint pixels, so the reduce is a plain sum). Tiles when params.batch < D:
    // the reference's default --batch 1 would leave all but one device idle under a sample split
    bool tile_split = false;
    float* red = nullptr;         // device 0: reduce target, W*H float4
    long long* red_hits = nullptr;
    std::vector<float> dn_host;   // the denoised image (jt_ctx::dn of a single-device context)
};

using namespace jtc;

namespace {

// RCCL, loaded on first use by a multi-device context (dlopen of the ROCm install's
// librccl.so.1): single-device contexts never touch it, and a process that already loaded an
// RCCL (e.g. torch's) shares that one instead of a second copy
struct Rccl {
    bool ok = false;
    decltype(&ncclCommInitAll) CommInitAll;
    decltype(&ncclCommDestroy) CommDestroy;
    decltype(&ncclReduce) Reduce;
    decltype(&ncclGroupStart) GroupStart;
    decltype(&ncclGroupEnd) GroupEnd;
    decltype(&ncclRedOpCreatePreMulSum) RedOpCreatePreMulSum;
    decltype(&ncclRedOpDestroy) RedOpDestroy;
    decltype(&ncclGetErrorString) GetErrorString;
};
const Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return x;
        x.CommInitAll = (decltype(x.CommInitAll))dlsym(h, "ncclCommInitAll");
        x.CommDestroy = (decltype(x.CommDestroy))dlsym(h, "ncclCommDestroy");
        x.Reduce = (decltype(x.Reduce))dlsym(h, "ncclReduce");
        x.GroupStart = (decltype(x.GroupStart))dlsym(h, "ncclGroupStart");
        x.GroupEnd = (decltype(x.GroupEnd))dlsym(h, "ncclGroupEnd");
        x.RedOpCreatePreMulSum = (decltype(x.RedOpCreatePreMulSum))dlsym(h, "ncclRedOpCreatePreMulSum");
        x.RedOpDestroy = (decltype(x.RedOpDestroy))dlsym(h, "ncclRedOpDestroy");
        x.GetErrorString = (decltype(x.GetErrorString))dlsym(h, "ncclGetErrorString");
        x.ok = x.CommInitAll && x.CommDestroy && x.Reduce && x.GroupStart && x.GroupEnd && x.RedOpCreatePreMulSum &&
               x.RedOpDestroy && x.GetErrorString;
        return x;
    }();
    return r;
}
int nccl_fail(ncclResult_t r, const char* what) {
    return jt::fail(JT_ERR_DEVICE, std::string(what) + ": " + rccl().GetErrorString(r));
}

// the reduce of the devices' running means onto device 0, then to the host. Sample split: one
// RCCL reduce with a per-rank premultiplied sum, sum_d mean_d * n_d / N; tile split: the devices'
// pixels are disjoint (zero elsewhere), so a plain sum. which: 0 image, 1 albedo, 2 normal
// (float4 buffers); hits (int64) are summed.
int multi_reduce(jt_ctx* c, int which, float* out4, int64_t* hits) {
    MultiCtx& m = *c->multi;
    const int D = (int)m.sub.size();
    const size_t np = (size_t)c->width * c->height;
    long long N = 0;
    for (long long n : m.nsub) N += n;
    // the premultiplied-sum ops created so far, destroyed on every exit path
    struct Ops {
        MultiCtx& m;
        std::vector<ncclRedOp_t> op;
        ~Ops() {
            for (size_t d = 0; d < op.size(); d++) (void)rccl().RedOpDestroy(op[d], m.comms[d]);
        }
    } ops{m, {}};
    std::vector<float> w(D);
    ncclResult_t r;
    if (out4 && !m.tile_split) {
        for (int d = 0; d < D; d++) {
            w[d] = N > 0 ? (float)((double)m.nsub[d] / (double)N) : (d == 0 ? 1.0f : 0.0f);
            ncclRedOp_t op;
            if ((r = rccl().RedOpCreatePreMulSum(&op, &w[d], ncclFloat32, ncclScalarHostImmediate, m.comms[d])) != ncclSuccess)
                return nccl_fail(r, "ncclRedOpCreatePreMulSum");
            ops.op.push_back(op);
        }
    }
    if ((r = rccl().GroupStart()) != ncclSuccess) return nccl_fail(r, "ncclGroupStart");
    for (int d = 0; d < D; d++) {
        jt_ctx* s = m.sub[d];
        (void)hipSetDevice(s->device);
        if (out4) {
            const float4* src = which == 0 ? s->A.image : which == 1 ? s->A.albedo : s->A.normal;
            r = rccl().Reduce(src, d == 0 ? (void*)m.red : (void*)src, np * 4, ncclFloat32,
                              m.tile_split ? ncclSum : ops.op[d], 0, m.comms[d], s->stream);
        } else {
            r = rccl().Reduce(s->A.hits, d == 0 ? (void*)m.red_hits : (void*)s->A.hits, np, ncclInt64, ncclSum, 0, m.comms[d],
                              s->stream);
        }
        if (r != ncclSuccess) {
            (void)rccl().GroupEnd();
            return nccl_fail(r, "ncclReduce");
        }
    }
    if ((r = rccl().GroupEnd()) != ncclSuccess) return nccl_fail(r, "ncclGroupEnd");
    hipError_t e;
    for (int d = 0; d < D; d++) {
        (void)hipSetDevice(m.sub[d]->device);
        if ((e = hipStreamSynchronize(m.sub[d]->stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    }
    (void)hipSetDevice(m.sub[0]->device);
    if (out4) e = hipMemcpy(out4, m.red, np * 16, hipMemcpyDeviceToHost);
    else e = hipMemcpy(hits, m.red_hits, np * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy reduce");
}

}  // namespace

extern "C" int jt_create_multi(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                               const int32_t* devices, int32_t ndevices, jt_ctx** out) {
    if (!out) return jt::fail(JT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!params) return jt::fail(JT_ERR_INVALID, "NULL argument");
    int avail = 0;
    if (hipGetDeviceCount(&avail) != hipSuccess) avail = 0;
    if (ndevices < 1 || ndevices > avail)
        return jt::fail(JT_ERR_INVALID, "ndevices must be in [1, " + std::to_string(avail) + "]");
    std::vector<int> devs(ndevices);
    for (int d = 0; d < ndevices; d++) {
        devs[d] = devices ? devices[d] : d;
        if (devs[d] < 0 || devs[d] >= avail) return jt::fail(JT_ERR_INVALID, "device id out of range");
        for (int k = 0; k < d; k++)
            if (devs[k] == devs[d]) return jt::fail(JT_ERR_INVALID, "a device is listed twice");
    }
    if (!rccl().ok) return jt::fail(JT_ERR_UNSUPPORTED, "librccl.so.1 (RCCL) could not be loaded");
    jt_ctx* c = new jt_ctx();
    c->multi = new MultiCtx();
    MultiCtx& m = *c->multi;
    for (int d = 0; d < ndevices; d++) {
        jt_params p = *params;
        p.device = devs[d];
        jt_ctx* s = nullptr;
        const int st = jt_create(scene, bvh, lights, &p, &s);
        if (st != JT_OK) {
            jt_destroy(c);
            return st;
        }
        m.sub.push_back(s);
    }
    m.nsub.assign(ndevices, 0);
    // split mode (MultiCtx::tile_split); the option multi_split=tiles|samples overrides
    m.tile_split = params->batch < ndevices;
    {
        const auto opts = jt::options_snapshot();
        const auto o = opts.find("multi_split");
        if (o != opts.end() && o->second == "tiles") m.tile_split = true;
        if (o != opts.end() && o->second == "samples") m.tile_split = false;
    }
    // every sub-context traces every tile under the sample split (a tile_share option never
    // leaves tiles out of the reduced image), its interleaved share under the tile split
    for (int d = 0; d < ndevices; d++) {
        m.sub[d]->P.tile_stride = m.tile_split ? ndevices : 1;
        m.sub[d]->P.tile_offset = m.tile_split ? d : 0;
        m.sub[d]->P.tile_stride_rcp = jtk::tile_stride_rcp(m.sub[d]->P.tile_stride);
        // a device's share leaves the other devices' tiles at zero for the summing reduce
        const int st = m.tile_split ? zero_if_stale(m.sub[d]) : JT_OK;
        if (st != JT_OK) {
            jt_destroy(c);
            return st;
        }
    }
    m.comms.resize(ndevices);
    ncclResult_t r = rccl().CommInitAll(m.comms.data(), ndevices, devs.data());
    if (r != ncclSuccess) {
        m.comms.clear();
        jt_destroy(c);
        return nccl_fail(r, "ncclCommInitAll");
    }
    jt_ctx* s0 = m.sub[0];
    c->device = s0->device;
    c->width = s0->width;
    c->height = s0->height;
    c->total_samples = s0->total_samples;
    c->batch = s0->batch;
    c->sampler = s0->sampler;
    c->lk = s0->lk;  // jt_get_streams: the devices' (fixed at jt_create)
    (void)hipSetDevice(s0->device);
    const size_t np = (size_t)c->width * c->height;
    if (hipMalloc(&m.red, np * 16) != hipSuccess || hipMalloc(&m.red_hits, np * 8) != hipSuccess) {
        jt_destroy(c);
        return jt::fail(JT_ERR_NOMEM, "hipMalloc reduce buffers");
    }
    *out = c;
    return JT_OK;
}

namespace jtc {

void multi_destroy(jt_ctx* c) {
    MultiCtx& m = *c->multi;
    for (ncclComm_t k : m.comms) (void)rccl().CommDestroy(k);
    if (!m.sub.empty()) {
        (void)hipSetDevice(m.sub[0]->device);
        if (m.red) (void)hipFree(m.red);
        if (m.red_hits) (void)hipFree(m.red_hits);
    }
    for (jt_ctx* s : m.sub) jt_destroy(s);
    delete c->multi;
    delete c;
}

int multi_reset(jt_ctx* c) {
    MultiCtx& m = *c->multi;
    for (jt_ctx* s : m.sub) {
        const int st = jt_reset(s);
        if (st != JT_OK) return st;
    }
    std::fill(m.nsub.begin(), m.nsub.end(), 0LL);
    c->pend0 = c->pend1 = 0;  // deferred samples are dropped with the state
    c->first = -1;
    c->next = 0;
    c->failed = false;
    c->launches = 0;
    c->kernel_ms = 0;
    return JT_OK;
}

// multi-device trace_samples step. Sample split: [s0, s1) in contiguous shares, one per device,
// each appended to that device's own running mean (weight 1/(n_d + k + 1) for its k-th new
// sample). Tile split: every device traces all of [s0, s1) on its own tiles (the running-mean
// weights are the single-device ones: first = the context's first sample).
int multi_trace_range(jt_ctx* c, int32_t s0, int32_t s1) {
    MultiCtx& m = *c->multi;
    const int D = (int)m.sub.size();
    std::vector<int> a(D, s0), b(D, s1);
    std::vector<char> launched(D, 0);
    int status = JT_OK;
    for (int d = 0; d < D && status == JT_OK; d++) {
        if (!m.tile_split) jtk::sample_share(s0, s1, d, D, &a[d], &b[d]);
        if (a[d] < b[d]) {
            const int32_t first = m.tile_split ? c->first : (int32_t)(a[d] - m.nsub[d]);
            status = trace_launch(m.sub[d], a[d], b[d], first);
            launched[d] = status == JT_OK;
        }
    }
    // wait for every launch already queued, even after a failed one: they add to their devices'
    // running means, so the context is unusable (failed) unless all of them ran
    float wall = 0;
    for (int d = 0; d < D; d++) {
        if (!launched[d]) continue;
        float ms = 0;
        const int st = trace_finish(m.sub[d], &ms);
        if (st != JT_OK && status == JT_OK) status = st;
        m.nsub[d] += b[d] - a[d];
        wall = std::max(wall, ms);
    }
    if (status != JT_OK) {
        c->failed = true;
        return status;
    }
    c->kernel_ms += wall;  // the launches run concurrently: the slowest device's time
    c->launches++;
    c->next = s1;
    return JT_OK;
}

int multi_get_image(jt_ctx* c, float* rgba) {
    for (jt_ctx* s : c->multi->sub)
        if (const int st = zero_if_stale(s)) return st;
    return multi_reduce(c, 0, rgba, nullptr);
}

int multi_get_aovs(jt_ctx* c, float* albedo, float* normal, int64_t* hits) {
    for (jt_ctx* s : c->multi->sub)
        if (const int st = zero_if_stale(s)) return st;
    for (jt_ctx* s : c->multi->sub)
        if (const int st = finish_aovs(s)) return st;
    std::vector<float4> tmp((size_t)c->width * c->height);
    int st;
    if (albedo) {
        if ((st = multi_reduce(c, 1, reinterpret_cast<float*>(tmp.data()), nullptr)) != JT_OK) return st;
        unpack3(tmp, albedo);
    }
    if (normal) {
        if ((st = multi_reduce(c, 2, reinterpret_cast<float*>(tmp.data()), nullptr)) != JT_OK) return st;
        unpack3(tmp, normal);
    }
    if (hits && (st = multi_reduce(c, 0, nullptr, hits)) != JT_OK) return st;
    return JT_OK;
}

// the devices' means reduced as jt_get_image / jt_get_aovs do, filtered on device 0
int multi_denoise(jt_ctx* c, const jt_denoise_params& p) {
    MultiCtx& m = *c->multi;
    const size_t np = (size_t)c->width * c->height;
    std::vector<float> img(np * 4), alb(np * 3), nrm(np * 3);
    int st;
    if ((st = jt_get_image(c, img.data())) || (st = jt_get_aovs(c, alb.data(), nrm.data(), nullptr))) return st;
    m.dn_host.resize(np * 4);
    if ((st = jt_denoise_image(img.data(), alb.data(), nrm.data(), c->width, c->height, &p, m.sub[0]->device, m.dn_host.data())))
        return st;
    c->denoised = true;
    return JT_OK;
}

int multi_get_denoised(jt_ctx* c, float* rgba) {
    std::memcpy(rgba, c->multi->dn_host.data(), (size_t)c->width * c->height * 16);
    return JT_OK;
}

// summed over the devices; kernel_ms: per launch the slowest device
int multi_get_counters(jt_ctx* c, jt_counters* out) {
    jt_counters sum{};
    for (jt_ctx* s : c->multi->sub) {
        jt_counters k{};
        const int st = jt_get_counters(s, &k);
        if (st != JT_OK) return st;
        sum.paths += k.paths;
        sum.rays += k.rays;
        sum.light_queries += k.light_queries;
        sum.nodes += k.nodes;
        sum.instances += k.instances;
        sum.prims += k.prims;
        sum.shades += k.shades;
    }
    sum.launches = c->launches;
    sum.kernel_ms = c->kernel_ms;
    *out = sum;
    return JT_OK;
}

// device 0's share; jt_trace_range then flushes every range at once (jt_ctx::exported)
int multi_get_device_buffers(jt_ctx* c, jt_device_buffers* out) {
    const int st = jt_get_device_buffers(c->multi->sub[0], out);
    if (st == JT_OK) c->exported = true;
    return st;
}

int multi_describe(const jt_ctx* c, char* buf, int32_t n) {
    const MultiCtx& m = *c->multi;
    char tmp[640];
    const int st = jt_describe(m.sub[0], tmp, sizeof tmp);
    if (st != JT_OK) return st;
    std::snprintf(buf, (size_t)n, "%s devices=%d split=%s", tmp, (int)m.sub.size(), m.tile_split ? "tiles" : "samples");
    return JT_OK;
}

int multi_set_counters(jt_ctx* c, int32_t level) {
    for (jt_ctx* s : c->multi->sub) s->count = level;
    c->count = level;
    return JT_OK;
}

int multi_synchronize(jt_ctx* c) {
    for (jt_ctx* s : c->multi->sub) {
        const int st = jt_synchronize(s);
        if (st != JT_OK) return st;
    }
    return JT_OK;
}

}  // namespace jtc
