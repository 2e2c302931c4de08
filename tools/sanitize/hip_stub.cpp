// A host-only stand-in for the HIP runtime entry points libpptoas_hip.so uses -- memory is malloc'ed, copies are
// memcpy's, kernels are NOT run, streams and events do nothing -- so that the library's HOST side (the worker thread
// of pp_fit_submit, the three-deep queue of pp_fit_enqueue / pp_fit_collect, staging blocks, deferred tails, the event
// pool) can run under ThreadSanitizer on a machine without a GPU:  LD_PRELOAD=libhip_stub.so ./tsan_driver
// (tools/sanitize/Makefile).  Not part of the product; nothing here computes a fit.
//
// PP_STUB_TRACE=<file>: one line per stream-visible call goes to that file -- kernel launches (device name, grid,
// block, dynamic LDS, stream), copies (kind, bytes, stream), memsets (value, bytes), event records and every wait or
// query, streams and events numbered in creation order -- which is what two builds of the host driver are compared
// by (trace_driver.cpp, make trace-run).  Allocations, frees, hipSetDevice, hipGetLastError and property queries are
// not logged.  Unset: nothing is written.
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

static std::atomic<long> g_launches{0}, g_allocs{0};
static thread_local struct { dim3 g, b; size_t sh; hipStream_t s; } t_cfg;

namespace {
struct Trace {
    std::mutex mu;
    FILE* f = nullptr;
    bool looked = false;
    std::map<const void*, std::string> kernels;   // host stub of a kernel -> its device name
    std::map<const void*, int> streams, events;   // handle -> ordinal in creation order (handles are recycled by malloc)
    int nstream = 0, nevent = 0;
};
Trace& tr() { static Trace* t = new Trace; return *t; }     // (never destroyed: the library's own teardown may log)
bool tracing(Trace& t) {
    if (!t.looked) {
        t.looked = true;
        const char* p = getenv("PP_STUB_TRACE");
        if (p && *p) t.f = fopen(p, "w");
    }
    return t.f != nullptr;
}
int ordinal(std::map<const void*, int>& m, const void* h) {
    if (!h) return 0;
    auto it = m.find(h);
    return it == m.end() ? -1 : it->second;
}
void logf(const char* fmt, ...) {
    Trace& t = tr();
    std::lock_guard<std::mutex> lk(t.mu);
    if (!tracing(t)) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(t.f, fmt, ap);
    va_end(ap);
    fputc('\n', t.f);
    fflush(t.f);
}
int stream_no(hipStream_t s) { Trace& t = tr(); std::lock_guard<std::mutex> lk(t.mu); return ordinal(t.streams, s); }
int event_no(hipEvent_t e) { Trace& t = tr(); std::lock_guard<std::mutex> lk(t.mu); return ordinal(t.events, e); }
const char* kind_name(hipMemcpyKind k) {
    switch (k) {
        case hipMemcpyHostToHost: return "H2H";
        case hipMemcpyHostToDevice: return "H2D";
        case hipMemcpyDeviceToHost: return "D2H";
        case hipMemcpyDeviceToDevice: return "D2D";
        default: return "default";
    }
}
hipError_t new_handle(void** h, bool is_stream) {
    *h = malloc(8);
    Trace& t = tr();
    std::lock_guard<std::mutex> lk(t.mu);
    if (is_stream) t.streams[*h] = ++t.nstream; else t.events[*h] = ++t.nevent;
    return hipSuccess;
}
}  // namespace

extern "C" {
long hip_stub_launches() { return g_launches.load(); }
// a comment line of the caller's into the trace (trace_driver.cpp names its cases with it)
void hip_stub_mark(const char* text) { logf("# %s", text); }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int) {
    memset(p, 0, sizeof *p);
    strcpy(p->name, "hip_stub");
    p->multiProcessorCount = 256; p->sharedMemPerBlock = 160 * 1024; p->totalGlobalMem = (size_t)288 << 30;
    p->warpSize = 64; p->maxThreadsPerBlock = 1024;
    strcpy(p->gcnArchName, "gfx950");
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) { ++g_allocs; *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemGetInfo(size_t* f, size_t* t) { *f = (size_t)200 << 30; *t = (size_t)288 << 30; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) {
    logf("memcpy %s %zu sync", kind_name(k), n);
    memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st) {
    logf("memcpy %s %zu s%d", kind_name(k), n, stream_no(st));
    memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t st) {
    logf("memcpy2d %s %zux%zu s%d", kind_name(k), w, h, stream_no(st));
    for (size_t r = 0; r < h; ++r) memmove((char*)d + r * dp, (const char*)s + r * sp, w);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) { logf("memset %d %zu sync", v, n); memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
    logf("memset %d %zu s%d", v, n, stream_no(st));
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return new_handle((void**)s, true); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return new_handle((void**)s, true); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t, const uint32_t*) { return new_handle((void**)s, true); }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t s) { logf("stream_query s%d", stream_no(s)); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { logf("stream_sync s%d", stream_no(s)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { logf("stream_wait s%d e%d", stream_no(s), event_no(e)); return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { return new_handle((void**)e, false); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return new_handle((void**)e, false); }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { logf("event_record e%d s%d", event_no(e), stream_no(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { logf("event_sync e%d", event_no(e)); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.01f; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = 2; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip_stub"; }
hipError_t hipLaunchKernel(const void* fn, dim3 g, dim3 b, void**, size_t sh, hipStream_t s) {
    ++g_launches;
    Trace& t = tr();
    std::string name;
    {
        std::lock_guard<std::mutex> lk(t.mu);
        if (tracing(t)) {
            auto it = t.kernels.find(fn);
            name = it == t.kernels.end() ? "?" : it->second;
        }
    }
    if (!name.empty()) logf("launch %s grid %u,%u,%u block %u,%u,%u lds %zu s%d", name.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, sh, stream_no(s));
    return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    Trace& t = tr();
    std::lock_guard<std::mutex> lk(t.mu);
    t.kernels[host_fn] = device_name ? device_name : "?";
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { t_cfg.g = g; t_cfg.b = b; t_cfg.sh = sh; t_cfg.s = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = t_cfg.g; *b = t_cfg.b; *sh = t_cfg.sh; *s = t_cfg.s; return hipSuccess; }
}
