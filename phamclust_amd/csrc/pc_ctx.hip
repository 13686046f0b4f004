// pc_ctx.hip -- the context of libphamclust_hip.so (include/phamclust_hip.h): error text and version, roctx ranges, device
// buffers, pc_ctx_create / pc_ctx_destroy, the tie rule and the small query and test hooks.
#include <cstdarg>
#include <cstdio>
#include <new>

#include "pc_host.h"

#include <dlfcn.h>

// roctx ranges around the stages of a fill (the reference only logs wall clock around matrix_de_novo).  The marker
// library is looked up at run time -- the product does not link against a profiler -- and the ranges show up in a
// `rocprofv3 --marker-trace` run as upload_sets / upload_residues / fill:<metric> / count / plan / align / reduce.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    Roctx() {
        if (getenv("PC_NO_ROCTX")) return;
        void* h = dlopen("libroctx64.so.4", RTLD_LAZY | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
static const Roctx& roctx() { static const Roctx r; return r; }
}  // namespace
PcRange::PcRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
PcRange::~PcRange() { if (on) roctx().pop(); }

static thread_local char g_err[512] = "";
void pc_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* pc_last_error(void) { return g_err; }
extern "C" int pc_version(void) { return PC_VERSION; }
extern "C" int pc_test_hooks(void) {
#ifdef PC_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
}

namespace {

// Fault injection (PC_FAKE_OOM_ABOVE=bytes): device allocations above that size made while a fill is planning fail, as if HBM
// were that small.  Compiled only under -DPC_TEST_HOOKS, i.e. into libphamclust_hip_hooks.so, the twin that
// test_out_of_memory_plan_becomes_smaller_chunks loads; the release library has no such switch (pc_test_hooks() tells which is which).
#ifdef PC_TEST_HOOKS
static thread_local bool g_planning = false;
static size_t fake_oom_limit() {
    static const size_t v = [] { const char* e = getenv("PC_FAKE_OOM_ABOVE"); return e ? (size_t)atoll(e) : (size_t)0; }();
    return g_planning ? v : 0;
}
#else
static constexpr size_t fake_oom_limit() { return 0; }
#endif
}  // namespace
#ifdef PC_TEST_HOOKS
PlanningScope::PlanningScope() { g_planning = true; }
PlanningScope::~PlanningScope() { g_planning = false; }
#else
PlanningScope::PlanningScope() {}
PlanningScope::~PlanningScope() {}
#endif

// Value injection (pc_hook_slab_values): the triangle a test sets stands for "the slab as filled" in every triangular slab walk of the
// process (slab_walk, pc_fill_slabs.hip) until it is cleared.  pc_hook_rows_values is its twin for the rows walk (rows_walk, the four rows
// forms): f64[n_rows][n], row k the values of the call's query genome rows[k], every element of every rows slab -- the diagonal and both
// copies of a pair of two query genomes included.  The two are independent: neither walk reads the other's.  The caller keeps the memory
// alive.  Set between calls only: the walks of a several-device fill read it from their own threads.  Compiled only under -DPC_TEST_HOOKS;
// the release library stores nothing and its getters answer NULL.
#ifdef PC_TEST_HOOKS
static const double* g_slab_values = nullptr;
static int64_t g_slab_n_pairs = 0;
static const double* g_rows_values = nullptr;
static int32_t g_rows_n_rows = 0, g_rows_n = 0;
const double* pc_hooked_slab_values(int64_t* n_pairs) { *n_pairs = g_slab_n_pairs; return g_slab_values; }
const double* pc_hooked_rows_values(int32_t* n_rows, int32_t* n) { *n_rows = g_rows_n_rows; *n = g_rows_n; return g_rows_values; }
extern "C" int pc_hook_slab_values(const double* values, int64_t n_pairs) {
    if (values && n_pairs < 0) { pc_set_error("pc_hook_slab_values: n_pairs %lld", (long long)n_pairs); return PC_ERR_ARG; }
    g_slab_values = values; g_slab_n_pairs = values ? n_pairs : 0;
    return PC_OK;
}
extern "C" int pc_hook_rows_values(const double* values, int32_t n_rows, int32_t n) {
    if (values && (n_rows < 0 || n < 0)) { pc_set_error("pc_hook_rows_values: n_rows %d, n %d", (int)n_rows, (int)n); return PC_ERR_ARG; }
    g_rows_values = values; g_rows_n_rows = values ? n_rows : 0; g_rows_n = values ? n : 0;
    return PC_OK;
}
#else
const double* pc_hooked_slab_values(int64_t* n_pairs) { *n_pairs = 0; return nullptr; }
const double* pc_hooked_rows_values(int32_t* n_rows, int32_t* n) { *n_rows = 0; *n = 0; return nullptr; }
extern "C" int pc_hook_slab_values(const double*, int64_t) {
    pc_set_error("pc_hook_slab_values: this library carries no test hooks (libphamclust_hip_hooks.so does)");
    return PC_ERR_STATE;
}
extern "C" int pc_hook_rows_values(const double*, int32_t, int32_t) {
    pc_set_error("pc_hook_rows_values: this library carries no test hooks (libphamclust_hip_hooks.so does)");
    return PC_ERR_STATE;
}
#endif

int DevBuf::ensure(size_t bytes) {
    if (bytes <= cap) return PC_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = (fake_oom_limit() && want > fake_oom_limit()) ? hipErrorOutOfMemory : hipMalloc(&p, want);
    if (e != hipSuccess) {
        pc_set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); p = nullptr; (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? PC_ERR_NOMEM_INTERNAL : PC_ERR_HIP;
    }
    cap = want; return PC_OK;
}

int PinnedBuf::ensure(size_t bytes) {
    if (bytes <= cap) return PC_OK;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    const size_t want = bytes + bytes / 8;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) { pc_set_error("hipHostMalloc(%zu): %s", want, hipGetErrorString(e)); p = nullptr; return PC_ERR_HIP; }
    cap = want; return PC_OK;
}

// For a result that is appended to over one call (pc_fill_edges): ensure() would drop what is already there.  Grows to twice the
// request so that a run of appends copies O(total) bytes.
int PinnedBuf::grow_keep(size_t bytes, size_t used) {
    if (bytes <= cap) return PC_OK;
    if (!p || used == 0) return ensure(bytes);
    void* q = nullptr;
    size_t want = bytes * 2;
    hipError_t e = hipHostMalloc(&q, want, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); want = bytes; e = hipHostMalloc(&q, want, hipHostMallocDefault); }   // (no room for the slack: the request alone)
    if (e != hipSuccess) { pc_set_error("hipHostMalloc(%zu): %s", want, hipGetErrorString(e)); (void)hipGetLastError(); return PC_ERR_HIP; }
    memcpy(q, p, used);
    (void)hipHostFree(p);
    p = q; cap = want;
    return PC_OK;
}

#ifndef PC_TIE_RULE_DEFAULT
#define PC_TIE_RULE_DEFAULT 0
#endif

extern "C" int pc_ctx_create(pc_ctx** out, int device_id) {
    if (!out) { pc_set_error("pc_ctx_create: out is NULL"); return PC_ERR_ARG; }
    *out = nullptr;
    int n = 0;
    PC_HIP(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) { pc_set_error("pc_ctx_create: device %d of %d", device_id, n); return PC_ERR_ARG; }
    pc_ctx* c = new (std::nothrow) pc_ctx();
    if (!c) { pc_set_error("out of host memory"); return PC_ERR_ARG; }
    c->device = device_id;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->n_cu = cus; }
    PcDeviceGuard guard(device_id);
    hipError_t e = guard.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming);
    if (const char* env = getenv("PC_PLAN_BYTES")) { const long long v = atoll(env); if (v > 0) c->plan_budget = v; }
    for (int i = 0; i < pc_ctx::kAux && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking);
    for (int i = 0; i <= pc_ctx::kAux && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->aux_ev[i], hipEventDisableTiming);
    if (const char* env = getenv("PC_ALIGN_STREAMS")) { int v = atoi(env); if (v >= 1 && v <= pc_ctx::kAux + 1) c->n_streams = v; }
    {
        int least = 0, greatest = 0;
        const char* env = getenv("PC_LONG_PRIORITY");
        const bool high = !(env && !strcmp(env, "0")) && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least;
        for (int i = 0; i < pc_ctx::kLong && e == hipSuccess; ++i) {
            if (high && hipStreamCreateWithPriority(&c->lng[i], hipStreamNonBlocking, greatest) != hipSuccess) { (void)hipGetLastError(); c->lng[i] = nullptr; }
            if (!c->lng[i]) e = hipStreamCreateWithFlags(&c->lng[i], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->lng_ev[i], hipEventDisableTiming);
        }
    }
    c->tie_rule = PC_TIE_RULE_DEFAULT;
    if (const char* env = getenv("PC_TIE_RULE")) { int v = atoi(env); if (v >= 0 && v < PC_NUM_TIE_RULES) c->tie_rule = v; }
    if (e != hipSuccess) { pc_set_error("pc_ctx_create: %s", hipGetErrorString(e)); pc_ctx_destroy(c); return PC_ERR_HIP; }
    if (c->h_plan.ensure(4096) != PC_OK) { pc_ctx_destroy(c); return PC_ERR_HIP; }
    *out = c;
    return PC_OK;
}

extern "C" void pc_ctx_destroy(pc_ctx* c) {
    if (!c) return;
    PcDeviceGuard guard(c->device);
    if (c->busy && c->ev_last) (void)hipEventSynchronize(c->ev_last);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < 5; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->ev_last) (void)hipEventDestroy(c->ev_last);
    for (hipEvent_t e : c->ev_slab) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < pc_ctx::kAux; ++i) if (c->aux[i]) { (void)hipStreamSynchronize(c->aux[i]); (void)hipStreamDestroy(c->aux[i]); }
    for (int i = 0; i <= pc_ctx::kAux; ++i) if (c->aux_ev[i]) (void)hipEventDestroy(c->aux_ev[i]);
    for (int i = 0; i < pc_ctx::kLong; ++i) {
        if (c->lng[i]) { (void)hipStreamSynchronize(c->lng[i]); (void)hipStreamDestroy(c->lng[i]); }
        if (c->lng_ev[i]) (void)hipEventDestroy(c->lng_ev[i]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                          // the buffers free themselves, still under the guard: on the context's device
}

extern "C" int pc_variant_width(int lb) {
    const int v = pc_nw_choose_variant(lb);
    return v < 0 ? 0 : pc_nw_variant_w(v);
}

extern "C" int pc_task_shape(int lb, int width, int32_t* out) {
    if (lb <= 0 || lb > 65535 || !out) { pc_set_error("pc_task_shape: bad argument"); return PC_ERR_ARG; }
    int v = -1;
    if (width == 0) v = pc_nw_choose_variant(lb);
    else for (int k = 0; k < pc_nw_num_variants(); ++k) if (pc_nw_variant_w(k) == width) v = k;
    if (v < 0) { pc_set_error("pc_task_shape: no systolic variant for w = %d, %d columns", width, lb); return PC_ERR_ARG; }
    const int W = pc_nw_variant_w(v);
    const bool strip = pc_nw_lanes(lb, W) > 64;
    out[0] = pc_nw_task_rows(lb, v, 0);
    out[1] = strip ? out[0] : pc_nw_class_waves(v, lb, 0);                   // strip-mined: one row per wave
    out[2] = pc_nw_segs(lb, W);                                             // (as pc_align_pairs cuts buckets)
    out[3] = strip ? pc_nw_strip_passes(lb, v) : 0;
    return PC_OK;
}
// The host cut of one bucket, from the functions the upload's tables and pc_align_pairs are made from (pc_bucket_cut): nothing
// here reads a device table or calls into pc_plan.hip, so a test can hold the device planner's counts against it.
extern "C" int pc_bucket_launch_classes(int lb, int rows, int any_byte, int32_t* out) {
    if (lb <= 0 || lb > 65535 || rows <= 0 || !out) { pc_set_error("pc_bucket_launch_classes: bad argument"); return PC_ERR_ARG; }
    const int base = pc_class_of(lb, pc_nw_choose_variant(lb), any_byte != 0);
    const PcBucketCut cut = pc_bucket_cut(lb, rows, base, any_byte != 0, true);
    const int last = (int)(cut.n_main % cut.per);
    out[0] = cut.per;
    out[1] = (int32_t)cut.n_main;
    out[2] = pc_task_launch_class(lb, cut.per, base, true);
    out[3] = last ? pc_task_launch_class(lb, last, base, true) : -1;
    out[4] = cut.rem_base >= 0 ? pc_task_launch_class(lb, (int)(rows - cut.n_main), cut.rem_base, true) : -1;
    return PC_OK;
}
extern "C" int pc_last_plan_tasks(const pc_ctx* c, int32_t* per_launch_class, int cap) {
    if (!c || cap < 0 || (cap > 0 && !per_launch_class)) { pc_set_error("pc_last_plan_tasks: bad argument"); return PC_ERR_ARG; }
    if (!c->last_plan_tasks_valid) { pc_set_error("pc_last_plan_tasks: no aai / peq fill on this context yet"); return PC_ERR_STATE; }
    const int n = (int)c->last_plan_tasks.size();
    for (int i = 0; i < n && i < cap; ++i) per_launch_class[i] = (int32_t)std::min<int64_t>(c->last_plan_tasks[i], INT32_MAX);
    return n;
}
extern "C" int pc_ppos_width(int max_lb) {
    int v = pc_nw_choose_variant(max_lb);                     // as run_align_classes' launch_variant picks it
    if (v >= 0 && !pc_nw_ppos_systolic(v, max_lb)) v = pc_nw_ppos_variant(max_lb);
    return v < 0 ? 0 : pc_nw_variant_w(v);
}

extern "C" float pc_last_align_ms(const pc_ctx* c) { return c ? c->last_align_ms : -1.f; }
extern "C" int pc_last_set_kernel(const pc_ctx* c) { return c ? c->last_set_kernel : -1; }

extern "C" int pc_set_tie_rule(pc_ctx* c, int rule) {
    if (!c) { pc_set_error("pc_set_tie_rule: NULL context"); return PC_ERR_ARG; }
    if (rule < 0 || rule >= PC_NUM_TIE_RULES) { pc_set_error("pc_set_tie_rule: rule %d not in 0..%d", rule, PC_NUM_TIE_RULES - 1); return PC_ERR_ARG; }
    c->tie_rule = rule;
    return PC_OK;
}
extern "C" int pc_get_tie_rule(const pc_ctx* c) { return c ? c->tie_rule : -1; }

// test hook for the device round(x, 6)
extern "C" int pc_round6_probe(pc_ctx* c, const double* in, double* out, int64_t n) {
    if (!c || n < 0) { pc_set_error("pc_round6_probe: bad argument"); return PC_ERR_ARG; }
    if (n == 0) return PC_OK;
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    DevBuf a, b;
    if ((rc = a.ensure(n * 8)) || (rc = b.ensure(n * 8))) return abi_rc(rc);
    hipError_t e = hipMemcpyAsync(a.p, in, n * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { rc = pc_launch_round6_probe(a.as<double>(), b.as<double>(), n, c->stream); }
    if (e == hipSuccess && rc == PC_OK) e = hipMemcpyAsync(out, b.p, n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { pc_set_error("pc_round6_probe: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return rc;
}
