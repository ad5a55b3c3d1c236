// capi_viewer.hip — a viewer frame lit and finished on the device (tbvh_sky_* / tbvh_viewer_*; include/tinybvh_amd.h, DESIGN.md par. 22): the rest of Trace and
// WorkerThread of tiny_bvh_gltf.cpp / tiny_bvh_foliage.cpp around the library's Intersect and GetShadingData.  A tbvh_sky owns a device copy of
// SkyDome::pixels; a tbvh_viewer owns a frame's buffers (ray records, shading records, colours, pixels, and — made by the first frame that needs them — the
// two queues of the alpha loop and the shadow rays) and renders into them on the context's stream: generate, { trace, shade } x rounds with the masked
// records compacted into a device-side queue, light, pack.  No round trip to the host: the queue's count stays in device memory (launchQuery's nDev).  The
// stage entry points launch one kernel each; the tbvh_host_* twins (viewer.h compiled for the host, no context) are in viewer_host.cpp.
#include "capi_internal.h"
#include "viewer_checks.h"

using namespace tbvh;
using namespace tbvh_capi;
using namespace tbvh_viewer_checks;

static_assert(kViewerGltf == TBVH_VIEWER_GLTF && kViewerFoliage == TBVH_VIEWER_FOLIAGE && kViewerMaxRounds == 8, "viewer.h and the public header agree");
static_assert(sizeof(tbvh_viewer_stats().rays) == kViewerMaxRounds * sizeof(uint64_t), "one ray count per round");

struct tbvh_sky {
    tbvh_context* ctx = nullptr;
    uint32_t width = 0, height = 0;
    DevBuf<float> pixels;
    ViewerSky view() const { return ViewerSky{pixels.get(), width, height}; }
};

struct tbvh_viewer {
    tbvh_context* ctx = nullptr;
    uint32_t width = 0, height = 0;
    uint64_t n = 0;
    DevBuf<float4> rays, out48, rgb;           // 4, 3 and 1 float4 per pixel
    DevBuf<uint32_t> pixels;
    DevBuf<float4> qRays[2], qOut48, shadow;   // the alpha loop's queues and the foliage mode's shadow rays: made by the first frame that needs them
    DevBuf<uint32_t> qPix[2];
    DevBuf<uint8_t> occ;
    DevBuf<unsigned long long> counters;       // [r]: records entering round r (r = 1 .. 7), [8]: shadow rays that are not null
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

namespace {

constexpr uint32_t kViewerCounters = 16;

int allocFail(const char* who, uint64_t bytes) {
    (void)hipGetLastError();
    return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)bytes);
}

template <class T>
int ensure(const char* who, DevBuf<T>& b, uint64_t count) {
    if (b.get()) return 0;
    return b.alloc(count) == hipSuccess ? 0 : allocFail(who, count * sizeof(T));
}

void destroySky(tbvh_sky* s) { delete s; }
void destroyViewer(tbvh_viewer* v) {
    tbvh_context* c = v->ctx;
    if (c->ev0 == v->e0 || c->ev1 == v->e1) { c->timed = false; c->ev0 = c->ev1 = nullptr; }   // (tbvh_time_last_ms pointed at this frame)
    if (v->e0) hipEventDestroy(v->e0);
    if (v->e1) hipEventDestroy(v->e1);
    delete v;
}

template <class T>
void unlist(std::vector<T*>& list, T* x) {
    for (size_t i = 0; i < list.size(); i++)
        if (list[i] == x) { list.erase(list.begin() + i); return; }
}

}  // namespace

namespace tbvh_capi {
void freeViewersOf(tbvh_context* c) {
    for (tbvh_viewer* v : c->viewers) destroyViewer(v);
    c->viewers.clear();
    for (tbvh_sky* s : c->skies) destroySky(s);
    c->skies.clear();
}
}  // namespace tbvh_capi

extern "C" {

// ---- the sky dome ---------------------------------------------------------------------------------------------------------------------------------------
int tbvh_sky_create(tbvh_context* c, const float* pixels12, uint32_t w, uint32_t h, int onDevice, tbvh_sky** out) {
    if (!c || !out || !pixels12) return fail(TBVH_E_INVALID, "tbvh_sky_create: null argument");
    if (int r = checkSkyHost("tbvh_sky_create", pixels12, w, h)) return r;
    TBVH_ENTER(c);
    tbvh_sky* s = new (std::nothrow) tbvh_sky;
    if (!s) return fail(TBVH_E_NOMEM, "tbvh_sky_create: out of host memory");
    s->ctx = c; s->width = w; s->height = h;
    const uint64_t words = 3ull * w * h;
    int r = 0;
    if (s->pixels.alloc(words) != hipSuccess) r = allocFail("tbvh_sky_create", words * 4);
    if (!r && hipMemcpyAsync(s->pixels, pixels12, words * 4, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream) != hipSuccess)
        r = fail(TBVH_E_HIP, "tbvh_sky_create: copying the texels failed: %s", hipGetErrorString(hipGetLastError()));
    const hipError_t e = hipStreamSynchronize(c->stream);   // (the caller's array is free from here on)
    if (!r && e != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_sky_create: %s", hipGetErrorString(e));
    if (r) { destroySky(s); return r; }
    c->skies.push_back(s);
    *out = s;
    return 0;
}

void tbvh_sky_free(tbvh_sky* s) {
    if (!s) return;
    tbvh_context* c = s->ctx;
    TBVH_LOCK(c);
    (void)tbvh_capi::setDevice(c);
    hipStreamSynchronize(c->stream);   // (kernels in flight read the texels)
    unlist(c->skies, s);
    destroySky(s);
}

int tbvh_sky_sample_device(tbvh_sky* s, const void* dDirs16, uint64_t n, void* dOut16) {
    if (!s) return fail(TBVH_E_INVALID, "tbvh_sky_sample_device: null sky");
    if (n && (!dDirs16 || !dOut16)) return fail(TBVH_E_INVALID, "tbvh_sky_sample_device: null directions or output");
    if (((uintptr_t)dDirs16 | (uintptr_t)dOut16) & 15) return fail(TBVH_E_INVALID, "tbvh_sky_sample_device: directions and output must be 16-byte aligned");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    launch_sky_sample(s->view(), dDirs16, n, dOut16, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the stages, one kernel each --------------------------------------------------------------------------------------------------------------------------
int tbvh_viewer_generate_device(tbvh_context* c, const tbvh_camera* cam, void* dRays64, uint64_t first, uint64_t n) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_viewer_generate_device: null context");
    ViewerCam vc;
    if (int r = checkCam("tbvh_viewer_generate_device", cam, &vc)) return r;
    if (first + n < first || first + n > (uint64_t)vc.width * vc.height) return fail(TBVH_E_INVALID, "tbvh_viewer_generate_device: rays %llu .. of a %u x %u image", (unsigned long long)first, vc.width, vc.height);
    if (int r = checkRecords("tbvh_viewer_generate_device", dRays64, 64, n)) return r;
    TBVH_ENTER(c);
    launch_viewer_generate(vc, dRays64, first, n, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_viewer_shadow_rays_device(tbvh_context* c, const void* dRays, uint32_t stride, uint64_t n, const float* lightDirOrNull, void* dShadow64) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_viewer_shadow_rays_device: null context");
    if (int r = checkRecords("tbvh_viewer_shadow_rays_device", dRays, stride, n)) return r;
    if (int r = checkRecords("tbvh_viewer_shadow_rays_device", dShadow64, 64, n)) return r;
    float L[3];
    lightDir(lightDirOrNull, L);
    TBVH_ENTER(c);
    launch_viewer_shadow_rays(dRays, stride, n, L, dShadow64, nullptr, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_viewer_light_device(tbvh_context* c, uint32_t mode, tbvh_shading* shadingOrNull, tbvh_sky* skyOrNull, const void* dRays, uint32_t stride, const void* dOut48,
                             const uint8_t* dOccOrNull, uint64_t n, const float* lightDirOrNull, void* dRgb16) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_viewer_light_device: null context");
    if (int r = checkMode("tbvh_viewer_light_device", mode)) return r;
    if (int r = checkRecords("tbvh_viewer_light_device", dRays, stride, n)) return r;
    if (n && (!dOut48 || !dRgb16)) return fail(TBVH_E_INVALID, "tbvh_viewer_light_device: null shading records or output");
    if (((uintptr_t)dOut48 | (uintptr_t)dRgb16) & 15) return fail(TBVH_E_INVALID, "tbvh_viewer_light_device: shading records and output must be 16-byte aligned");
    if ((skyOrNull && skyOrNull->ctx != c) || (shadingOrNull && shadingContext(shadingOrNull) != c))
        return fail(TBVH_E_INVALID, "tbvh_viewer_light_device: the sky or the shading table belongs to another context");
    float L[3];
    lightDir(lightDirOrNull, L);
    TBVH_ENTER(c);
    launch_viewer_light(mode, skyOrNull ? skyOrNull->view() : ViewerSky{nullptr, 0, 0}, dRays, stride, dOut48, dOccOrNull, n, L, dRgb16, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_viewer_pack_device(tbvh_context* c, const void* dRgb16, uint64_t n, uint32_t* dPixels) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_viewer_pack_device: null context");
    if (n && (!dRgb16 || !dPixels)) return fail(TBVH_E_INVALID, "tbvh_viewer_pack_device: null colours or pixels");
    if (((uintptr_t)dRgb16 & 15) || ((uintptr_t)dPixels & 3)) return fail(TBVH_E_INVALID, "tbvh_viewer_pack_device: misaligned colours (16 bytes) or pixels (4)");
    TBVH_ENTER(c);
    launch_viewer_pack(dRgb16, n, dPixels, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the frame ------------------------------------------------------------------------------------------------------------------------------------------
int tbvh_viewer_create(tbvh_context* c, uint32_t w, uint32_t h, tbvh_viewer** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_viewer_create: null argument");
    if (w == 0 || h == 0 || (uint64_t)w * h >> 31) return fail(TBVH_E_INVALID, "tbvh_viewer_create: a %u x %u image (positive, below 2^31 pixels in all)", w, h);
    TBVH_ENTER(c);
    tbvh_viewer* v = new (std::nothrow) tbvh_viewer;
    if (!v) return fail(TBVH_E_NOMEM, "tbvh_viewer_create: out of host memory");
    v->ctx = c; v->width = w; v->height = h; v->n = (uint64_t)w * h;
    hipError_t e = v->rays.alloc(4 * v->n);
    if (e == hipSuccess) e = v->out48.alloc(3 * v->n);
    if (e == hipSuccess) e = v->rgb.alloc(v->n);
    if (e == hipSuccess) e = v->pixels.alloc(v->n);
    if (e == hipSuccess) e = v->counters.alloc(kViewerCounters);
    if (e == hipSuccess) e = hipEventCreate(&v->e0);
    if (e == hipSuccess) e = hipEventCreate(&v->e1);
    if (e != hipSuccess) { (void)hipGetLastError(); destroyViewer(v); return fail(TBVH_E_NOMEM, "tbvh_viewer_create: %s", hipGetErrorString(e)); }
    c->viewers.push_back(v);
    *out = v;
    return 0;
}

void tbvh_viewer_destroy(tbvh_viewer* v) {
    if (!v) return;
    tbvh_context* c = v->ctx;
    TBVH_LOCK(c);
    (void)tbvh_capi::setDevice(c);
    hipStreamSynchronize(c->stream);
    unlist(c->viewers, v);
    destroyViewer(v);
}

int tbvh_viewer_render(tbvh_viewer* v, tbvh_scene* s, tbvh_shading* sh, tbvh_sky* skyOrNull, const tbvh_camera* cam, const tbvh_viewer_params* p, tbvh_viewer_stats* stats) {
    if (!v || !s || !sh || !p) return fail(TBVH_E_INVALID, "tbvh_viewer_render: null argument");
    TBVH_REFUSE_DOUBLE(s, "tbvh_viewer_render");
    TBVH_REFUSE_VOXEL(s, "tbvh_viewer_render");
    TBVH_REFUSE_CUSTOM(s, "tbvh_viewer_render");
    tbvh_context* c = v->ctx;
    if (s->ctx != c || shadingContext(sh) != c || (skyOrNull && skyOrNull->ctx != c))
        return fail(TBVH_E_INVALID, "tbvh_viewer_render: the viewer, the scene, the shading table and the sky must belong to one context");
    if (int r = checkMode("tbvh_viewer_render", p->mode)) return r;
    if (p->max_rounds > kViewerMaxRounds) return fail(TBVH_E_INVALID, "tbvh_viewer_render: %u rounds (1 .. 8, or 0 for 8)", p->max_rounds);
    if (p->flags) return fail(TBVH_E_INVALID, "tbvh_viewer_render: flags %u (none are defined)", p->flags);
    ViewerCam vc;
    if (int r = checkCam("tbvh_viewer_render", cam, &vc)) return r;
    if (vc.width != v->width || vc.height != v->height)
        return fail(TBVH_E_INVALID, "tbvh_viewer_render: a %u x %u camera on a %u x %u viewer", vc.width, vc.height, v->width, v->height);
    float L[3];
    lightDir(p->light_dir, L);
    const ShadeMat* mats; uint32_t nMats, nTex; bool anyColorTex;
    shadingMaterials(sh, &mats, &nMats, &nTex, &anyColorTex);
    // the foliage viewer never continues (its `#if 1`), nor does a table without colour textures: both known here
    const uint32_t rounds = p->mode == TBVH_VIEWER_GLTF && anyColorTex ? (p->max_rounds ? p->max_rounds : kViewerMaxRounds) : 1u;
    const uint64_t n = v->n;
    TBVH_ENTER(c);
    if (rounds > 1) {
        for (int k = 0; k < 2; k++) {
            if (int r = ensure("tbvh_viewer_render", v->qRays[k], 4 * n)) return r;
            if (int r = ensure("tbvh_viewer_render", v->qPix[k], n)) return r;
        }
        if (int r = ensure("tbvh_viewer_render", v->qOut48, 3 * n)) return r;
    }
    if (p->mode == TBVH_VIEWER_FOLIAGE) {
        if (int r = ensure("tbvh_viewer_render", v->shadow, 4 * n)) return r;
        if (int r = ensure("tbvh_viewer_render", v->occ, n)) return r;
    }
    hipStream_t st = c->stream;
    HIP_TRY(hipEventRecord(v->e0, st));
    HIP_TRY(hipMemsetAsync(v->counters, 0, kViewerCounters * sizeof(unsigned long long), st));
    launch_viewer_generate(vc, v->rays, 0, n, st);
    // one event pair brackets the FRAME (e0 / e1: tbvh_viewer_stats::frame_ms, tbvh_time_last_ms), not every query of it, as the wavefront frame does
    struct Untimed { tbvh_context* c; bool was; ~Untimed() { c->skipTiming = was; } } untimed{c, c->skipTiming};
    c->skipTiming = true;
    // round 0 goes out with the size the host knows: probed, sampled by the scene's schedule tuner and traced by the kernel it settles on (no slot in the probe
    // memory: the frame's launches carry no events of their own)
    if (int r = launchQuery(s, (RayRec*)v->rays.get(), n, nullptr)) return r;
    shadingLaunch(sh, s, v->rays, n, 64, v->out48, nullptr);
    if (rounds > 1) launch_viewer_compact(v->rays, v->out48, n, mats, nMats, nTex, v->qRays[0], v->qPix[0], v->counters.get() + 1, st);
    for (uint32_t r = 1; r < rounds; r++) {
        const int cur = (int)(r - 1) & 1, nxt = cur ^ 1;
        const unsigned long long* count = v->counters.get() + r;
        if (int e = launchQuery(s, (RayRec*)v->qRays[cur].get(), n, nullptr, false, 1e30f, count)) return e;
        shadingLaunch(sh, s, v->qRays[cur], n, 64, v->qOut48, count);
        launch_viewer_requeue(v->qRays[cur], v->qPix[cur], v->qOut48, count, n, mats, nMats, nTex, r + 1 == rounds, v->qRays[nxt], v->qPix[nxt], v->counters.get() + r + 1, v->rays,
                              v->out48, st);
    }
    const uint8_t* occ = nullptr;
    if (p->mode == TBVH_VIEWER_FOLIAGE) {
        launch_viewer_shadow_rays(v->rays, 64, n, L, v->shadow, v->counters.get() + 8, st);
        if (int e = launchQuery(s, (RayRec*)v->shadow.get(), n, v->occ)) return e;
        occ = v->occ;
    }
    launch_viewer_light(p->mode, skyOrNull ? skyOrNull->view() : ViewerSky{nullptr, 0, 0}, v->rays, 64, v->out48, occ, n, L, v->rgb, st);
    launch_viewer_pack(v->rgb, n, v->pixels, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(v->e1, st));
    c->ev0 = v->e0; c->ev1 = v->e1; c->timed = true;   // tbvh_time_last_ms: the frame (destroying the viewer withdraws the pair)
    if (stats) {
        unsigned long long h[kViewerCounters];
        HIP_TRY(hipMemcpyAsync(h, v->counters, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memset(stats, 0, sizeof *stats);
        stats->rays[0] = n;
        for (uint32_t r = 1; r < rounds; r++) stats->rays[r] = h[r];
        stats->shadow_rays = h[8];
        HIP_TRY(hipEventElapsedTime(&stats->frame_ms, v->e0, v->e1));
        if (int r = checkStatus(c)) return r;
    }
    return 0;
}

int tbvh_viewer_read_pixels(tbvh_viewer* v, uint32_t* pixels) {
    if (!v || !pixels) return fail(TBVH_E_INVALID, "tbvh_viewer_read_pixels: null argument");
    tbvh_context* c = v->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(pixels, v->pixels, v->n * 4, hipMemcpyDeviceToHost, c->stream));
    return checkStatus(c);   // (synchronizes)
}

int tbvh_viewer_read_rgb(tbvh_viewer* v, void* rgb16) {
    if (!v || !rgb16) return fail(TBVH_E_INVALID, "tbvh_viewer_read_rgb: null argument");
    tbvh_context* c = v->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(rgb16, v->rgb, v->n * 16, hipMemcpyDeviceToHost, c->stream));
    return checkStatus(c);
}

int tbvh_viewer_rays(tbvh_viewer* v, void** dRays64) {
    if (!v || !dRays64) return fail(TBVH_E_INVALID, "tbvh_viewer_rays: null argument");
    *dRays64 = v->rays.get();
    return 0;
}

}  // extern "C"
