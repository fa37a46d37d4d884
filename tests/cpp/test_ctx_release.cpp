// Host program over the C-ABI of libss_hip.so (tests/test_gpu_ctx_release.py builds and runs it on a GPU): does a context, with every
// form it prepares lazily, give back to the HIP runtime everything it took — on the success paths and when a creation fails?
//
// The program defines the runtime's allocation and release calls itself (the executable's definitions come first in symbol lookup, so
// the library's calls arrive here), forwards them to the runtime (dlsym RTLD_NEXT) and keeps a ledger: what is live, and that nothing
// is released twice or without having been handed out.  Each phase drives the ABI with host arrays at the smallest shapes at which
// its part exists, checks that the form it is there for actually ran, destroys its context and requires an empty ledger.  The
// creation phases refuse the k-th allocation of a create, for every k, without calling the runtime.
//   (no argument)  every phase; one line "PHASE <name> ok" or "PHASE <name> FAILED: <why>" each, "CREATE_FAIL <entry> <k> <message>"
//   --dump         the same run, and every phase's sequence of (call, bytes)
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ss_hip.h"

// ---- the ledger ---------------------------------------------------------------------------------------------------------------
namespace {

std::mutex g_mu;                                   // (the reserve thread allocates beside the caller's thread)
std::map<void*, const char*> g_live;               // handle -> the call that handed it out
std::vector<std::string> g_wrong;                  // releases the ledger does not know, or knows as released
std::vector<std::string> g_calls, g_calls_other;   // the phase's takes: by the caller's thread in order, by other threads
std::thread::id g_main;
long g_allocs = 0;                                 // hipMalloc + hipHostMalloc calls since the last reset
long g_fail_at = -1;                               // the one of them that is refused (-1: none)
long g_streams = 0, g_events = 0;

template <typename F> F next(const char* name)
{
    void* f = dlsym(RTLD_NEXT, name);
    if (!f) { std::fprintf(stderr, "no %s behind this program\n", name); std::abort(); }
    return reinterpret_cast<F>(f);
}

void note_take(const char* call, void* h, size_t bytes)
{
    char line[96];
    std::snprintf(line, sizeof(line), "%s %zu", call, bytes);
    std::lock_guard<std::mutex> lock(g_mu);
    (std::this_thread::get_id() == g_main ? g_calls : g_calls_other).push_back(line);
    if (g_live.count(h)) g_wrong.push_back(std::string(call) + ": handed out a handle that is live");
    g_live[h] = call;
}

// false: not ours to forward (already released, or never handed out)
bool note_release(const char* call, void* h)
{
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_live.find(h);
    if (it == g_live.end()) { g_wrong.push_back(std::string(call) + ": released twice or never handed out"); return false; }
    g_live.erase(it);
    return true;
}

bool refuse_this_one()
{
    std::lock_guard<std::mutex> lock(g_mu);
    return g_allocs++ == g_fail_at;
}

}  // namespace

extern "C" {

hipError_t hipMalloc(void** p, size_t bytes)
{
    static auto real = next<hipError_t (*)(void**, size_t)>("hipMalloc");
    if (refuse_this_one()) { *p = nullptr; return hipErrorOutOfMemory; }
    const hipError_t e = real(p, bytes);
    if (e == hipSuccess && *p) note_take("hipMalloc", *p, bytes);
    return e;
}
hipError_t hipFree(void* p)
{
    static auto real = next<hipError_t (*)(void*)>("hipFree");
    if (!p) return real(p);
    return note_release("hipFree", p) ? real(p) : hipErrorInvalidValue;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags)
{
    static auto real = next<hipError_t (*)(void**, size_t, unsigned int)>("hipHostMalloc");
    if (refuse_this_one()) { *p = nullptr; return hipErrorOutOfMemory; }
    const hipError_t e = real(p, bytes, flags);
    if (e == hipSuccess && *p) note_take("hipHostMalloc", *p, bytes);
    return e;
}
hipError_t hipHostFree(void* p)
{
    static auto real = next<hipError_t (*)(void*)>("hipHostFree");
    if (!p) return real(p);
    return note_release("hipHostFree", p) ? real(p) : hipErrorInvalidValue;
}
hipError_t hipEventCreate(hipEvent_t* e)
{
    static auto real = next<hipError_t (*)(hipEvent_t*)>("hipEventCreate");
    const hipError_t r = real(e);
    if (r == hipSuccess) { note_take("hipEventCreate", *e, 0); g_events += 1; }
    return r;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    static auto real = next<hipError_t (*)(hipEvent_t*, unsigned)>("hipEventCreateWithFlags");
    const hipError_t r = real(e, flags);
    if (r == hipSuccess) { note_take("hipEventCreateWithFlags", *e, 0); g_events += 1; }
    return r;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    static auto real = next<hipError_t (*)(hipEvent_t)>("hipEventDestroy");
    return note_release("hipEventDestroy", e) ? real(e) : hipErrorInvalidValue;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int flags)
{
    static auto real = next<hipError_t (*)(hipStream_t*, unsigned int)>("hipStreamCreateWithFlags");
    const hipError_t r = real(s, flags);
    if (r == hipSuccess) { note_take("hipStreamCreateWithFlags", *s, 0); g_streams += 1; }
    return r;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int flags, int priority)
{
    static auto real = next<hipError_t (*)(hipStream_t*, unsigned int, int)>("hipStreamCreateWithPriority");
    const hipError_t r = real(s, flags, priority);
    if (r == hipSuccess) { note_take("hipStreamCreateWithPriority", *s, 0); g_streams += 1; }
    return r;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    static auto real = next<hipError_t (*)(hipStream_t)>("hipStreamDestroy");
    return note_release("hipStreamDestroy", s) ? real(s) : hipErrorInvalidValue;
}

}  // extern "C"

// ---- phases -------------------------------------------------------------------------------------------------------------------
namespace {

bool g_dump = false;
int g_failed = 0;

struct Phase {
    std::string name, why;
    explicit Phase(const std::string& n) : name(n)
    {
        std::lock_guard<std::mutex> lock(g_mu);
        g_calls.clear(); g_calls_other.clear(); g_wrong.clear();
        g_allocs = 0; g_fail_at = -1; g_streams = 0; g_events = 0;
        if (!g_live.empty()) why = "the ledger was not empty when the phase began";
    }
    void need(bool cond, const char* fmt, ...)
    {
        if (cond || !why.empty()) return;
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        why = buf;
    }
    // after the phase's context is destroyed
    void end()
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (why.empty() && !g_wrong.empty()) why = g_wrong[0];
        if (why.empty() && !g_live.empty()) {
            std::map<std::string, int> by;
            for (auto& kv : g_live) by[kv.second] += 1;
            why = "not given back:";
            for (auto& kv : by) why += " " + std::to_string(kv.second) + " x " + kv.first;
        }
        g_live.clear();
        if (why.empty()) std::printf("PHASE %s ok\n", name.c_str());
        else { std::printf("PHASE %s FAILED: %s\n", name.c_str(), why.c_str()); g_failed += 1; }
        if (g_dump) {
            for (auto& c : g_calls) std::printf("DUMP %s %s\n", name.c_str(), c.c_str());
            for (auto& c : g_calls_other) std::printf("DUMP %s (other thread) %s\n", name.c_str(), c.c_str());
        }
        std::fflush(stdout);
    }
};

long takes_so_far() { std::lock_guard<std::mutex> lock(g_mu); return (long)(g_calls.size() + g_calls_other.size()); }

// a small generator: the same numbers on every machine
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 1) {}
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
    double gauss() { double a = 0; for (int i = 0; i < 12; ++i) a += uni(); return a - 6.0; }
};

// A [m][n] row-major with columns of about unit norm; B signals, each a combination of k columns with coefficients in 1 .. 2
template <typename T> struct Problem {
    size_t m, n, B;
    std::vector<T> A, Y;
    Problem(size_t m_, size_t n_, size_t B_, size_t k, uint64_t seed) : m(m_), n(n_), B(B_), A(m_ * n_), Y(B_ * m_)
    {
        Rng r(seed);
        const double sc = 1.0 / std::sqrt((double)m);
        for (auto& a : A) a = (T)(r.gauss() * sc);
        for (size_t b = 0; b < B; ++b) {
            std::vector<double> y(m, 0.0);
            for (size_t t = 0; t < k; ++t) {
                const size_t j = (size_t)(r.uni() * (double)n) % n;
                const double c = 1.0 + r.uni();
                for (size_t i = 0; i < m; ++i) y[i] += c * (double)A[i * n + j];
            }
            for (size_t i = 0; i < m; ++i) Y[b * m + i] = (T)y[i];
        }
    }
};

char g_err[512];

// the entry points by element type
inline ss_hip_ctx* create(const float* A, size_t m, size_t n) { return ss_hip_homotopy_create_f32(A, m, n, (ptrdiff_t)n, 1, 0, g_err, sizeof(g_err)); }
inline ss_hip_ctx* create(const double* A, size_t m, size_t n) { return ss_hip_homotopy_create_f64(A, m, n, (ptrdiff_t)n, 1, 0, g_err, sizeof(g_err)); }
inline ss_hip_ctx* irls_create(const float* A, size_t m, size_t n) { return ss_hip_irls_create_f32(A, m, n, (ptrdiff_t)n, 1, 0, g_err, sizeof(g_err)); }
inline ss_hip_ctx* irls_create(const double* A, size_t m, size_t n) { return ss_hip_irls_create_f64(A, m, n, (ptrdiff_t)n, 1, 0, g_err, sizeof(g_err)); }
#define BY_TYPE(name) template <typename... A> int name(const float*, A... a) { return name##_f32(a...); } \
                      template <typename... A> int name(const double*, A... a) { return name##_f64(a...); }
BY_TYPE(ss_hip_homotopy_solve) BY_TYPE(ss_hip_homotopy_solve_batch) BY_TYPE(ss_hip_homotopy_solve_batch_compact) BY_TYPE(ss_hip_omp_solve_batch)
BY_TYPE(ss_hip_class_residuals) BY_TYPE(ss_hip_refit_records) BY_TYPE(ss_hip_nonneg_refit_records) BY_TYPE(ss_hip_top_correlations)
BY_TYPE(ss_hip_nonneg_top_correlations) BY_TYPE(ss_hip_extend_records) BY_TYPE(ss_hip_group_top_correlations) BY_TYPE(ss_hip_group_class_residuals)
BY_TYPE(ss_hip_weighted_top_correlations) BY_TYPE(ss_hip_weighted_refit_records) BY_TYPE(ss_hip_weighted_class_residuals) BY_TYPE(ss_hip_robust_weights)
BY_TYPE(ss_hip_homotopy_atom_update) BY_TYPE(ss_hip_homotopy_ksvd_sweep) BY_TYPE(ss_hip_weighted_atom_update) BY_TYPE(ss_hip_atom_coherence)
BY_TYPE(ss_hip_irls_solve) BY_TYPE(ss_hip_irls_solve_batch) BY_TYPE(ss_hip_homotopy_colshard_solve)
#undef BY_TYPE
inline ss_hip_ctx* colshard_create(const float* A, size_t m, size_t n)
{ return ss_hip_homotopy_colshard_create_f32(A, m, n, (ptrdiff_t)n, 1, 0, n, 0, nullptr, 0, 1, nullptr, g_err, sizeof(g_err)); }
inline ss_hip_ctx* colshard_create(const double* A, size_t m, size_t n)
{ return ss_hip_homotopy_colshard_create_f64(A, m, n, (ptrdiff_t)n, 1, 0, n, 0, nullptr, 0, 1, nullptr, g_err, sizeof(g_err)); }

ss_hip_stats stats_of(ss_hip_ctx* ctx) { ss_hip_stats s; std::memset(&s, 0, sizeof(s)); (void)ss_hip_get_stats(ctx, &s); return s; }
#define OK(ph, call) do { g_err[0] = 0; const int rc_ = (call); (ph).need(rc_ == SS_HIP_OK, "%s returned %d: %s", #call, rc_, g_err); } while (0)

template <typename T> const T* tag() { return nullptr; }

// ---- fp32 Homotopy, 1000 x 512: the screened solve, the regrow, the batch forms, G and its reserve thread
void phase_f32_forms()
{
    typedef float T;
    Phase ph("homotopy_f32_1000x512");
    const size_t m = 1000, n = 512, B = 8;
    Problem<T> P(m, n, B, 6, 1);
    ss_hip_ctx* ctx = create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        std::vector<T> X(B * n);
        std::vector<uint32_t> it(B);
        std::vector<double> er(B);
        OK(ph, ss_hip_set_option(ctx, "screen_single", 2));
        OK(ph, ss_hip_set_option(ctx, "trace", 1));
        ss_hip_stats s0 = stats_of(ctx);
        OK(ph, ss_hip_homotopy_solve(tag<T>(), ctx, P.Y.data(), 1, (T)1e-3, 40u, X.data(), 1, it.data(), er.data(), g_err, sizeof(g_err)));
        ss_hip_stats s1 = stats_of(ctx);
        ph.need(s1.screen_signals > s0.screen_signals, "the single solve did not run in the screened form");
        ph.need(s1.screen_resident > s0.screen_resident, "the screened solve's path did not run in the resident kernel");
        // max_iterations = 200: the workspace (19 arrays) and the Gram-column cache are taken anew
        long t0 = takes_so_far();
        OK(ph, ss_hip_homotopy_solve(tag<T>(), ctx, P.Y.data() + m, 1, (T)1e-3, 200u, X.data(), 1, it.data(), er.data(), g_err, sizeof(g_err)));
        ph.need(takes_so_far() - t0 >= 19 + 5, "the second solve did not regrow the workspace and the cache (%ld takes)", takes_so_far() - t0);
        // a batch of 8 without G
        s0 = stats_of(ctx);
        OK(ph, ss_hip_homotopy_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 40u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), g_err, sizeof(g_err)));
        s1 = stats_of(ctx);
        ph.need(s1.gram_full_builds == s0.gram_full_builds, "the first batch formed G");
        ph.need(it[0] > 0 && it[B - 1] > 0, "the batch without G reported no iterations");
        // batch_gram_min = 4: the reserve thread, G, the subset form (batch_min = 4: a batch of 8 counts as one that runs in lock-step)
        OK(ph, ss_hip_set_option(ctx, "batch_gram_min", 4));
        OK(ph, ss_hip_set_option(ctx, "batch_min", 4));
        OK(ph, ss_hip_homotopy_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 40u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), g_err, sizeof(g_err)));
        ss_hip_stats s2 = stats_of(ctx);
        ph.need(s2.gram_full_builds == s1.gram_full_builds + 1, "the batch of 8 under batch_gram_min = 4 did not form G");
        ph.need(s2.subset_signals > s1.subset_signals, "the batch on G did not run in the subset form");
        // an OMP batch on G (tracing off from here: a traced OMP batch runs one signal at a time and makes no Gram-form buffers)
        OK(ph, ss_hip_set_option(ctx, "trace", 0));
        OK(ph, ss_hip_omp_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 12u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), g_err, sizeof(g_err)));
        ss_hip_stats s3 = stats_of(ctx);
        ph.need(s3.omp_gram_signals > s2.omp_gram_signals, "the OMP batch did not run in the Gram form");
        // a compact batch
        const uint32_t kmax = 16;
        const size_t rb = ss_hip_record_bytes(kmax, 0);
        std::vector<uint64_t> recs(B * rb / 8);
        OK(ph, ss_hip_homotopy_solve_batch_compact(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 40u, kmax, recs.data(), g_err, sizeof(g_err)));
        ph.need((uint32_t)recs[0] > 0u, "the compact batch wrote an empty record");
        // the reference-order engine
        OK(ph, ss_hip_set_option(ctx, "engine", 3));
        OK(ph, ss_hip_homotopy_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 40u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), g_err, sizeof(g_err)));
        ph.need(it[0] > 0, "the reference-order batch reported no iterations");
        ss_hip_homotopy_destroy(ctx);
    }
    ph.end();
}

// ---- fp32 Homotopy, 256 x 16896: the early form (n > 16384) makes streams 2 - 4, their events and the per-SE counters
void phase_f32_early()
{
    typedef float T;
    Phase ph("homotopy_f32_256x16896_early");
    const size_t m = 256, n = 16896;
    Problem<T> P(m, n, 1, 6, 2);
    ss_hip_ctx* ctx = create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        std::vector<T> x(n);
        uint32_t it = 0;
        double er = 0;
        OK(ph, ss_hip_set_option(ctx, "screen_single", 0));
        const ss_hip_stats s0 = stats_of(ctx);
        OK(ph, ss_hip_homotopy_solve(tag<T>(), ctx, P.Y.data(), 1, (T)1e-3, 24u, x.data(), 1, &it, &er, g_err, sizeof(g_err)));
        const ss_hip_stats s1 = stats_of(ctx);
        ph.need(s1.solo_solves > s0.solo_solves, "the solve did not run in the speculative form");
        ph.need(g_streams >= 3, "the early form made no further streams (%ld in all)", g_streams);
        ss_hip_homotopy_destroy(ctx);
    }
    ph.end();
}

// ---- fp32: G reserved by the helper thread but never formed
void phase_f32_reserved()
{
    typedef float T;
    Phase ph("homotopy_f32_reserved_never_formed");
    const size_t m = 64, n = 512, B = 4;
    Problem<T> P(m, n, B, 4, 3);
    ss_hip_ctx* ctx = create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        std::vector<T> X(B * n);
        std::vector<uint32_t> it(B);
        std::vector<double> er(B);
        OK(ph, ss_hip_homotopy_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 16u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), g_err, sizeof(g_err)));
        ph.need(stats_of(ctx).gram_full_builds == 0, "the batch of 4 formed G");
        ss_hip_homotopy_destroy(ctx);       // (joins the thread)
        const size_t gbytes = (size_t)512 * 1024 * sizeof(float);
        bool reserved = false;
        { std::lock_guard<std::mutex> lock(g_mu); for (auto& c : g_calls_other) reserved = reserved || c == "hipMalloc " + std::to_string(gbytes); }
        ph.need(reserved, "no helper thread reserved G's %zu bytes", gbytes);
    }
    ph.end();
}

// ---- fp64 Homotopy, 256 x 8192: the sub-context with its state log, the resident tier's batch buffers
void phase_f64_screened()
{
    typedef double T;
    Phase ph("homotopy_f64_256x8192_screened");
    const size_t m = 256, n = 8192, B = 4;
    Problem<T> P(m, n, B, 6, 4);
    ss_hip_ctx* ctx = create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        std::vector<T> X(B * n);
        std::vector<uint32_t> it(B);
        std::vector<double> er(B);
        OK(ph, ss_hip_set_option(ctx, "screen_single", 2));
        const ss_hip_stats s0 = stats_of(ctx);
        OK(ph, ss_hip_homotopy_solve(tag<T>(), ctx, P.Y.data(), 1, (T)1e-6, 24u, X.data(), 1, it.data(), er.data(), g_err, sizeof(g_err)));
        const ss_hip_stats s1 = stats_of(ctx);
        ph.need(s1.screen_signals > s0.screen_signals, "the fp64 solve did not run in the screened form");
        ph.need(g_streams >= 2, "no sub-context was made (%ld streams)", g_streams);
        OK(ph, ss_hip_homotopy_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-6, 24u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), g_err, sizeof(g_err)));
        const ss_hip_stats s2 = stats_of(ctx);
        ph.need(s2.screen_signals > s1.screen_signals && s2.screen_resident > s1.screen_resident, "the fp64 batch did not run in the resident tier");
        bool batch_buffers = false;      // (Screen64Batch's signals in fp16: [128][ldm] halves)
        { std::lock_guard<std::mutex> lock(g_mu); for (auto& c : g_calls) batch_buffers = batch_buffers || c == "hipMalloc " + std::to_string((size_t)128 * 256 * 2); }
        ph.need(batch_buffers, "the fp64 batch made no chunk buffers");
        ss_hip_homotopy_destroy(ctx);
    }
    ph.end();
}

// ---- the record calls, 70 x 200, B = 8, kmax = 5
template <typename T> void phase_records(const char* name)
{
    Phase ph(name);
    const size_t m = 70, n = 200, B = 8, S = 4, C = 4, Gn = 2;
    const uint32_t kmax = 5, k = 3;
    Problem<T> P(m, n, B, 3, 5);
    ss_hip_ctx* ctx = create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        const T* Y = P.Y.data();
        const ptrdiff_t ys = (ptrdiff_t)m;
        const size_t rb = ss_hip_record_bytes(kmax, sizeof(T) == 8);
        std::vector<uint64_t> recs(B * rb / 8), out(B * rb / 8);
        std::vector<uint32_t> labels(n), best(B), status(B), dropped(B), idx(B * k), added(B), usage(S), partner(S), cols(S);
        std::vector<uint32_t> goff = { 0u, 3u, (uint32_t)B };
        std::vector<T> R(B * C), coef(B * k), W(B * m, (T)1), Wout(B * m), V(m * S);
        std::vector<double> sci(B), resnorm(B), score(B * k), objective(2), mu(S), scale(B);
        for (size_t j = 0; j < n; ++j) labels[j] = (uint32_t)(j % C);
        for (size_t s = 0; s < S; ++s) cols[s] = (uint32_t)(s * 7);
        OK(ph, ss_hip_homotopy_solve_batch_compact(tag<T>(), ctx, Y, B, ys, 1, (T)1e-3, 4u, kmax, recs.data(), g_err, sizeof(g_err)));
        ph.need((uint32_t)recs[0] >= 1u && (uint32_t)recs[0] <= kmax, "the first record does not hold its support (K = %u)", (unsigned)(uint32_t)recs[0]);
        OK(ph, ss_hip_set_classes(ctx, labels.data(), (uint32_t)C, g_err, sizeof(g_err)));
        OK(ph, ss_hip_class_residuals(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, R.data(), (ptrdiff_t)C, best.data(), sci.data(), g_err, sizeof(g_err)));
        ph.need(best[0] < C, "class residuals: no class for the first signal");
        OK(ph, ss_hip_refit_records(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, out.data(), resnorm.data(), status.data(), g_err, sizeof(g_err)));
        ph.need(status[0] == SS_HIP_REFIT_DONE, "refit: status %u", status[0]);
        OK(ph, ss_hip_nonneg_refit_records(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, out.data(), resnorm.data(), status.data(), dropped.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_top_correlations(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, k, idx.data(), coef.data(), score.data(), g_err, sizeof(g_err)));
        ph.need(idx[0] < n, "top correlations: no column for the first signal");
        OK(ph, ss_hip_extend_records(tag<T>(), ctx, recs.data(), B, kmax, idx.data(), coef.data(), k, out.data(), added.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_nonneg_top_correlations(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, k, idx.data(), coef.data(), score.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_group_top_correlations(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, goff.data(), Gn, k, idx.data(), coef.data(), score.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_group_class_residuals(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, goff.data(), Gn, R.data(), (ptrdiff_t)C, best.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_weighted_top_correlations(tag<T>(), ctx, Y, B, ys, 1, W.data(), (ptrdiff_t)m, recs.data(), kmax, 0.0, k, idx.data(), coef.data(), score.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_weighted_refit_records(tag<T>(), ctx, Y, B, ys, 1, W.data(), (ptrdiff_t)m, recs.data(), kmax, out.data(), resnorm.data(), status.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_weighted_class_residuals(tag<T>(), ctx, Y, B, ys, 1, W.data(), (ptrdiff_t)m, recs.data(), kmax, R.data(), (ptrdiff_t)C, best.data(), sci.data(), g_err, sizeof(g_err)));
        OK(ph, ss_hip_robust_weights(tag<T>(), ctx, Y, B, ys, 1, (const T*)nullptr, (ptrdiff_t)0, recs.data(), kmax, (uint32_t)SS_HIP_ROBUST_HUBER, 1.345, 0.0, Wout.data(), (ptrdiff_t)m,
                                     (T*)nullptr, (ptrdiff_t)0, scale.data(), g_err, sizeof(g_err)));
        ph.need(scale[0] == scale[0], "robust weights: the first scale is NaN");
        OK(ph, ss_hip_homotopy_atom_update(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, cols.data(), S, V.data(), (ptrdiff_t)S, (ptrdiff_t)1, usage.data(), objective.data(), 0u, g_err, sizeof(g_err)));
        OK(ph, ss_hip_homotopy_ksvd_sweep(tag<T>(), ctx, Y, B, ys, 1, recs.data(), kmax, out.data(), cols.data(), S, V.data(), (ptrdiff_t)S, (ptrdiff_t)1, usage.data(), objective.data(), 0u, g_err, sizeof(g_err)));
        OK(ph, ss_hip_weighted_atom_update(tag<T>(), ctx, Y, B, ys, 1, W.data(), (ptrdiff_t)m, recs.data(), kmax, out.data(), cols.data(), S, V.data(), (ptrdiff_t)S, (ptrdiff_t)1, usage.data(),
                                           objective.data(), 0u, g_err, sizeof(g_err)));
        OK(ph, ss_hip_atom_coherence(tag<T>(), ctx, cols.data(), S, mu.data(), partner.data(), g_err, sizeof(g_err)));
        ph.need(mu[0] == mu[0], "coherence: NaN for the first atom");
        ss_hip_homotopy_destroy(ctx);
    }
    ph.end();
}

// ---- IRLS 64 x 16: a solve and a batch of 3
template <typename T> void phase_irls(const char* name)
{
    Phase ph(name);
    const size_t m = 64, n = 16, B = 3;
    Problem<T> P(m, n, B, 3, 6);
    ss_hip_ctx* ctx = irls_create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        std::vector<T> X(B * n);
        std::vector<uint32_t> it(B);
        std::vector<double> er(B);
        std::vector<int> spd(B);
        OK(ph, ss_hip_irls_solve(tag<T>(), ctx, P.Y.data(), 1, (T)1e-3, 10u, X.data(), 1, it.data(), er.data(), spd.data(), g_err, sizeof(g_err)));
        ph.need(it[0] > 0, "the IRLS solve reported no iterations");
        const long t0 = takes_so_far();
        OK(ph, ss_hip_irls_solve_batch(tag<T>(), ctx, P.Y.data(), B, (ptrdiff_t)m, 1, (T)1e-3, 10u, X.data(), (ptrdiff_t)n, 1, it.data(), er.data(), spd.data(), g_err, sizeof(g_err)));
        ph.need(it[B - 1] > 0 && takes_so_far() - t0 >= 6, "the IRLS batch made no workspace (%ld takes)", takes_so_far() - t0);
        ss_hip_irls_destroy(ctx);
    }
    ph.end();
}

// ---- column-sharded, world 1, no transport: two solves on one context, the second with a larger max_iterations
template <typename T> void phase_colshard(const char* name)
{
    Phase ph(name);
    const size_t m = 64, n = 256;
    Problem<T> P(m, n, 2, 4, 7);
    ss_hip_ctx* ctx = colshard_create(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    if (ctx) {
        std::vector<T> x(n);
        uint32_t it = 0;
        double er = 0;
        const T tol = sizeof(T) == 8 ? (T)1e-6 : (T)1e-3;
        OK(ph, ss_hip_homotopy_colshard_solve(tag<T>(), ctx, P.Y.data(), 1, tol, 20u, x.data(), 1, &it, &er, g_err, sizeof(g_err)));
        ph.need(it > 0, "the first sharded solve reported no iterations");
        const long t0 = takes_so_far();
        OK(ph, ss_hip_homotopy_colshard_solve(tag<T>(), ctx, P.Y.data() + m, 1, tol, 100u, x.data(), 1, &it, &er, g_err, sizeof(g_err)));
        ph.need(it > 0 && takes_so_far() - t0 >= 14, "the second sharded solve did not regrow the replicated active set (%ld takes)", takes_so_far() - t0);
        ss_hip_homotopy_destroy(ctx);
    }
    ph.end();
}

// ---- a creation whose k-th allocation is refused: null with a message, nothing kept, and the next creation succeeds
template <typename T, typename Create> void phase_failed_create(const char* name, Create make, size_t m, size_t n)
{
    Phase ph(name);
    Problem<T> P(m, n, 1, 2, 8);
    ss_hip_ctx* ctx = make(P.A.data(), m, n);
    ph.need(ctx != nullptr, "create: %s", g_err);
    long total = 0;
    { std::lock_guard<std::mutex> lock(g_mu); total = g_allocs; }
    ss_hip_homotopy_destroy(ctx);
    for (long kth = 0; kth < total && ctx; ++kth) {
        size_t live_before = 0;
        { std::lock_guard<std::mutex> lock(g_mu); g_allocs = 0; g_fail_at = kth; live_before = g_live.size(); }
        g_err[0] = 0;
        ss_hip_ctx* bad = make(P.A.data(), m, n);
        { std::lock_guard<std::mutex> lock(g_mu); g_fail_at = -1; ph.need(g_live.size() == live_before, "allocation %ld refused: %zu handles kept", kth, g_live.size() - live_before); }
        ph.need(bad == nullptr, "allocation %ld refused: create returned a context", kth);
        ph.need(g_err[0] != 0, "allocation %ld refused: no message", kth);
        std::printf("CREATE_FAIL %s %ld %s\n", name, kth, g_err);
        if (bad) ss_hip_homotopy_destroy(bad);
        ss_hip_ctx* good = make(P.A.data(), m, n);
        ph.need(good != nullptr, "the create after refusal %ld failed: %s", kth, g_err);
        ss_hip_homotopy_destroy(good);
    }
    ph.end();
}

}  // namespace

int main(int argc, char** argv)
{
    g_main = std::this_thread::get_id();
    g_dump = argc > 1 && std::strcmp(argv[1], "--dump") == 0;
    if (ss_hip_device_count() < 1) { std::printf("no HIP device\n"); return 2; }
    phase_f32_forms();
    phase_f32_early();
    phase_f32_reserved();
    phase_f64_screened();
    phase_records<float>("records_f32");
    phase_records<double>("records_f64");
    phase_irls<float>("irls_f32");
    phase_irls<double>("irls_f64");
    phase_colshard<float>("colshard_f32");
    phase_colshard<double>("colshard_f64");
    phase_failed_create<float>("homotopy_create_f32", [](const float* A, size_t m, size_t n) { return create(A, m, n); }, 64, 32);
    phase_failed_create<double>("homotopy_create_f64", [](const double* A, size_t m, size_t n) { return create(A, m, n); }, 64, 32);
    phase_failed_create<float>("irls_create_f32", [](const float* A, size_t m, size_t n) { return irls_create(A, m, n); }, 64, 16);
    phase_failed_create<double>("irls_create_f64", [](const double* A, size_t m, size_t n) { return irls_create(A, m, n); }, 64, 16);
    std::printf(g_failed ? "%d phase(s) failed\n" : "all phases passed\n", g_failed);
    return g_failed ? 1 : 0;
}
