// abi.hip -- the C ABI of include/cofhe_hip.h, in this order: the context, the block cache, the entry helpers (the overlap
// test, the piece grid, spans, the checked launch and its two-build form, flag words, the table-cache lookup), the workspace plans, the launchers (one launch site per kernel and
// route; product_tree is the pairwise tree of them all) and the host-side tensor formats.  The kernels are declared in
// kernels.hpp and defined in cofhe_hip.hip, wide.hip, comb.hip, affine.hip, matmul_left.hip, conv.hip, conv_ct.hip, pow_dot.hip,
// divide.hip, divide_exact.hip, lut.hip, spline.hip, view.hip and compare.hip; this file holds no device code of its own.  conv.hip holds the three kernels of the
// convolution, conv_ct.hip the two that ciphertext filters add, pow_dot.hip the two of
// the polynomial evaluation, divide.hip the signed floor division of the division by public divisors, divide_exact.hip the four
// kernels of the exact division by small divisors, lut.hip the two copies of
// the table lookups, spline.hip the three kernels of the piecewise-polynomial activations, view.hip the two that rearrange
// resident tensors, compare.hip the two of the digit comparisons.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../../include/cofhe_hip.h"
#include "ctx.hpp"
#include "form_io.hpp"
#include "kernels.hpp"
#include "conv.hpp"
#include "plain_mm.hpp"
#include "poly_shift.hpp"
#include "plain_div.hpp"
#include "plain_divmod.hpp"
#include "lut.hpp"
#include "spline.hpp"
#include "view.hpp"
#include "compare.hpp"

using namespace cofhe;
using namespace cofhe_k;

namespace {

// ---- little-endian limb strings (host): the context reads its discriminant with these, the formats section its tensors
size_t sig_bytes(const uint8_t *p, size_t n) {
    while (n > 0 && p[n - 1] == 0) n--;
    return n;
}

size_t bits_of(const uint32_t *w, int words) {
    for (int i = words - 1; i >= 0; i--)
        if (w[i]) return (size_t)i * 32 + 32 - __builtin_clz(w[i]);
    return 0;
}

}  // namespace

// ---- the host side of the fixed-base comb: per context, its cached tables and its two option pins ----------------------
// A side table keyed by the context pointer, not members of cofhe_hip_ctx: ctx.hpp is one of the files the kernel code hash reads.
// The two option pins of the convolution live here for the same reason.
namespace {
struct CombTable {
    uint32_t base[REC_WORDS];
    uint32_t w = 0;
    uint32_t *d = nullptr;
    uint64_t stamp = 0;
};
struct CombState {
    static constexpr int N_TABLES = 8;           // w = 10: 100 x 512 records = 34.4 MB each
    CombTable tabs[N_TABLES];
    uint64_t clock = 0;
    uint32_t opt_width = 0;                      // "comb_width": 0 = the launcher decides
    uint64_t opt_chunk = 0;                      // "comb_chunk": 0 = the launcher decides
    uint32_t opt_conv_route = 0;                 // "conv_route": 0 = the launcher decides, 1 direct wherever it does not decline, 2 gather
    uint32_t opt_conv_chunk_rows = 0;            // "conv_chunk_rows": 0 = the launcher decides, else rows per chunk of the direct route
    uint32_t opt_view_grid_blocks = 0;           // "view_grid_blocks": 0 = the launcher decides, else the grid of k_view_records and k_gather_records
};
std::mutex g_comb_mu;
std::unordered_map<const cofhe_hip_ctx *, CombState *> g_comb;
CombState &comb_state(const cofhe_hip_ctx *ctx) {
    std::lock_guard<std::mutex> lk(g_comb_mu);
    CombState *&st = g_comb[ctx];
    if (!st) st = new CombState();
    return *st;
}
void comb_release(const cofhe_hip_ctx *ctx) {
    CombState *st = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_comb_mu);
        auto it = g_comb.find(ctx);
        if (it == g_comb.end()) return;
        st = it->second;
        g_comb.erase(it);
    }
    for (auto &t : st->tabs)
        if (t.d) (void)hipFree(t.d);
    delete st;
}
}  // namespace

extern "C" {

const char *cofhe_hip_last_error(void) { return g_err.c_str(); }
int cofhe_hip_record_words(void) { return REC_WORDS; }
int cofhe_hip_exp_words(void) { return EXP_MAG_WORDS; }
void cofhe_hip_host_free(void *p) { free(p); }

int cofhe_hip_ctx_create(int device, const uint8_t *absdelta_le, size_t len, cofhe_hip_ctx **out) {
    if (!out || !absdelta_le) return fail(COFHE_HIP_EINVAL, "null argument");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(COFHE_HIP_EHIP, "no such HIP device (the engine has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    size_t n = sig_bytes(absdelta_le, len);
    if (n == 0 || n > 2 * PLIMBS * 4) return fail(COFHE_HIP_EINVAL, "discriminant out of range");
    std::vector<uint32_t> dl(2 * PLIMBS + 1, 0);
    memcpy(dl.data(), absdelta_le, n);
    const int dbits = (int)bits_of(dl.data(), 2 * PLIMBS);
    // capacity: reduced a, b < 2^(dbits/2) must leave headroom in one 1280-bit plane
    if (dbits > 2400) return fail(COFHE_HIP_EINVAL, "discriminant above 2400 bits is not supported by the 40-limb planes");
    const uint32_t mod4 = (4u - (dl[0] & 3u)) & 3u;     // Delta mod 4 from |Delta|
    if (mod4 != 0 && mod4 != 1) return fail(COFHE_HIP_EINVAL, "Delta must be 0 or 1 mod 4");
    // principal form (1, b0, (b0 - Delta)/4)
    std::vector<uint32_t> one(REC_WORDS, 0);
    one[REC_A] = 1;
    one[REC_B] = mod4;
    {   // c = (b0 + |Delta|) / 4
        uint64_t carry = mod4;
        std::vector<uint32_t> t(2 * PLIMBS + 1, 0);
        for (int i = 0; i < 2 * PLIMBS + 1; i++) {
            uint64_t s = (uint64_t)dl[i] + carry;
            t[i] = (uint32_t)s;
            carry = s >> 32;
        }
        for (int i = 0; i < 2 * PLIMBS; i++) one[REC_C + i] = (t[i] >> 2) | (t[i + 1] << 30);
    }
    cofhe_hip_ctx *c = new cofhe_hip_ctx();
    c->device = device;
    c->dbits = dbits;
    c->half_dbits = (dbits + 1) / 2;
    hipError_t e = hipMalloc((void **)&c->d_one, (REC_WORDS + 2 * PLIMBS + 4 + cofhe_hip_ctx::N_FLAGS) * 4);
    if (e != hipSuccess) {
        delete c;
        return fail(COFHE_HIP_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    c->d_absdelta = c->d_one + REC_WORDS;
    c->d_status = c->d_absdelta + 2 * PLIMBS;
    c->d_flags = c->d_status + 4;
    e = hipMemset(c->d_status, 0, 16);
    if (e == hipSuccess) e = hipMemcpy(c->d_absdelta, dl.data(), 2 * PLIMBS * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_one, one.data(), REC_WORDS * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(c->d_one);
        delete c;
        return fail(COFHE_HIP_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    {   // block cache limit: an eighth of the device memory, at most 64 GiB (cofhe_hip_trim changes it)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b / 8 < c->pool_cap) c->pool_cap = total_b / 8;
    }
    *out = c;
    return COFHE_HIP_OK;
}

static void pool_release_all(cofhe_hip_ctx *ctx);
void cofhe_hip_ctx_destroy(cofhe_hip_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipFree(ctx->d_one);
    if (ctx->workspace) hipFree(ctx->workspace);
    if (ctx->ws_event) (void)hipEventDestroy(ctx->ws_event);
    if (ctx->d_ftab) hipFree(ctx->d_ftab);
    for (auto &e : ctx->fb)
        if (e.d_table) hipFree(e.d_table);
    comb_release(ctx);
    (void)hipDeviceSynchronize();
    for (auto &sp : ctx->prof) {
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    pool_release_all(ctx);
    delete ctx;
}

// Allocation goes through a per-context cache of freed blocks (exact rounded size): hipFree synchronises the whole
// device and hipMalloc costs ~100 us, which dominated chains of small tensor operations.  A freed block carries an
// event recorded on the null stream (ordered after everything submitted to it and to blocking streams); taking the
// block out again waits for that event on the host, normally long past.
static void pool_release_all(cofhe_hip_ctx *ctx) {
    for (auto &kv : ctx->pool) {
        (void)hipEventDestroy(kv.second.ev);
        (void)hipFree(kv.second.p);
    }
    ctx->pool.clear();
    ctx->pooled_bytes = 0;
}
// hipMalloc that gives the context's cached blocks back to the driver and retries when the device is out of memory:
// the cache may hold up to pool_cap bytes that nobody is using
static hipError_t dev_alloc(cofhe_hip_ctx *ctx, void **dptr, size_t bytes) {
    hipError_t e = hipMalloc(dptr, bytes);
    if (e == hipErrorOutOfMemory && !ctx->pool.empty()) {
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
        pool_release_all(ctx);
        e = hipMalloc(dptr, bytes);
    }
    return e;
}
int cofhe_hip_malloc(cofhe_hip_ctx *ctx, size_t bytes, void **dptr) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    // size classes: multiples of 512 B up to 4 KiB, above that eighths of the power of two below the request (at most
    // 12.5 % slack), so that buffers of slightly different lengths (serialised tensors) share cached blocks
    size_t sz = ((bytes ? bytes : 4) + 511) & ~(size_t)511;
    if (sz > 4096) {
        size_t p2 = (size_t)1 << (63 - __builtin_clzll((unsigned long long)sz));
        const size_t step = p2 / 8;
        sz = (sz + step - 1) / step * step;
    }
    auto it = ctx->pool.find(sz);
    if (it != ctx->pool.end()) {
        const cofhe_hip_ctx::Pooled b = it->second;
        ctx->pool.erase(it);
        ctx->pooled_bytes -= sz;
        HIPCHK(hipEventSynchronize(b.ev));
        (void)hipEventDestroy(b.ev);
        *dptr = b.p;
        ctx->live[b.p] = sz;
        return COFHE_HIP_OK;
    }
    HIPCHK(dev_alloc(ctx, dptr, sz));
    ctx->live[*dptr] = sz;
    return COFHE_HIP_OK;
}
int cofhe_hip_free(cofhe_hip_ctx *ctx, void *dptr) { return cofhe_hip_free_on_stream(ctx, dptr, nullptr); }
int cofhe_hip_free_on_stream(cofhe_hip_ctx *ctx, void *dptr, void *stream) {
    if (!dptr) return COFHE_HIP_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    auto it = ctx->live.find(dptr);
    if (it == ctx->live.end()) {            // not one of ours
        HIPCHK(hipFree(dptr));
        return COFHE_HIP_OK;
    }
    const size_t sz = it->second;
    ctx->live.erase(it);
    if (ctx->pooled_bytes + sz > ctx->pool_cap) {
        HIPCHK(hipFree(dptr));
        return COFHE_HIP_OK;
    }
    cofhe_hip_ctx::Pooled b{dptr, nullptr};
    HIPCHK(hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
    // the event orders the block's reuse after the work already queued on `stream` (the stream the block was last used
    // on; the null stream also covers every blocking stream)
    HIPCHK(hipEventRecord(b.ev, (hipStream_t)stream));
    ctx->pool.emplace(sz, b);
    ctx->pooled_bytes += sz;
    return COFHE_HIP_OK;
}
int cofhe_hip_ctx_set_option(cofhe_hip_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return fail(COFHE_HIP_EINVAL, "null argument");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const std::string n(name);
    if (n == "wnaf_width") {
        if (value != 0 && (value < 2 || value > 8)) return fail(COFHE_HIP_EINVAL, "wnaf_width: 0 (automatic) or 2..8");
        ctx->opt_wnaf_width = (uint32_t)value;
    } else if (n == "matmul_segments") {
        if (value < 0 || value > (1 << 20)) return fail(COFHE_HIP_EINVAL, "matmul_segments: 0 (automatic) or a positive count");
        ctx->opt_matmul_segments = (uint32_t)value;
    } else if (n == "ladder_form") {
        if (value < 0 || value > 4)
            return fail(COFHE_HIP_EINVAL, "ladder_form: 0 (automatic), 1 (wide, two wavefronts), 2 (solo), 3 (throughput kernel), 4 (wide, one wavefront)");
        ctx->opt_ladder_form = (int)value;
    } else if (n == "matmul_tree") {
        if (value < -1 || value > 1) return fail(COFHE_HIP_EINVAL, "matmul_tree: -1 (automatic), 0 (chains) or 1 (product tree)");
        ctx->opt_matmul_tree = (int)value;
    } else if (n == "profile_kernels") {
        ctx->opt_profile = value != 0;
    } else if (n == "comb_width") {
        if (value != 0 && (value < COMB_W_MIN || value > COMB_W_MAX)) return fail(COFHE_HIP_EINVAL, "comb_width: 0 (automatic) or 2..10");
        comb_state(ctx).opt_width = (uint32_t)value;
    } else if (n == "comb_chunk") {
        if (value < 0 || value > (1ll << 32)) return fail(COFHE_HIP_EINVAL, "comb_chunk: 0 (automatic) or a positive count");
        comb_state(ctx).opt_chunk = (uint64_t)value;
    } else if (n == "conv_route") {
        if (value < 0 || value > 2) return fail(COFHE_HIP_EINVAL, "conv_route: 0 (automatic), 1 (direct) or 2 (gather)");
        comb_state(ctx).opt_conv_route = (uint32_t)value;
    } else if (n == "conv_chunk_rows") {
        if (value < 0 || value > 0xFFFFFFFFll) return fail(COFHE_HIP_EINVAL, "conv_chunk_rows: 0 (automatic) or a positive count");
        comb_state(ctx).opt_conv_chunk_rows = (uint32_t)value;
    } else if (n == "view_grid_blocks") {
        if (value < 0 || value > (1 << 20)) return fail(COFHE_HIP_EINVAL, "view_grid_blocks: 0 (automatic) or a workgroup count up to 2^20");
        comb_state(ctx).opt_view_grid_blocks = (uint32_t)value;
    } else {
        return fail(COFHE_HIP_EINVAL, "unknown option: " + n);
    }
    return COFHE_HIP_OK;
}
int cofhe_hip_profile_read(cofhe_hip_ctx *ctx, const char *kernel, float *total_ms, uint32_t *launches, int clear) {
    if (!ctx || !kernel || !total_ms) return fail(COFHE_HIP_EINVAL, "null argument");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    float sum = 0;
    uint32_t cnt = 0;
    for (auto &sp : ctx->prof) {
        if (strcmp(sp.name, kernel) != 0) continue;
        HIPCHK(hipEventSynchronize(sp.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, sp.a, sp.b));
        sum += ms;
        cnt++;
    }
    *total_ms = sum;
    if (launches) *launches = cnt;
    if (clear) {
        for (auto &sp : ctx->prof) {
            (void)hipEventDestroy(sp.a);
            (void)hipEventDestroy(sp.b);
        }
        ctx->prof.clear();
    }
    return COFHE_HIP_OK;
}
int cofhe_hip_trim(cofhe_hip_ctx *ctx, size_t keep_bytes) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->pool_cap = keep_bytes;
    if (ctx->pooled_bytes > keep_bytes) {
        HIPCHK(hipDeviceSynchronize());
        pool_release_all(ctx);
    }
    return COFHE_HIP_OK;
}
int cofhe_hip_upload(cofhe_hip_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return COFHE_HIP_OK;
}
int cofhe_hip_download(cofhe_hip_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return COFHE_HIP_OK;
}
int cofhe_hip_stream_sync(cofhe_hip_ctx *ctx, void *stream) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return COFHE_HIP_OK;
}
// A stream of the library's own HIP runtime on the context's device: what a client that shares one context among worker
// threads gives each of them (a handle of another runtime in the process, PyTorch's for one, means nothing here).
int cofhe_hip_stream_create(cofhe_hip_ctx *ctx, int nonblocking, void **stream) {
    if (!ctx || !stream) return fail(COFHE_HIP_EINVAL, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, nonblocking ? hipStreamNonBlocking : hipStreamDefault));
    *stream = (void *)s;
    return COFHE_HIP_OK;
}
int cofhe_hip_stream_destroy(cofhe_hip_ctx *ctx, void *stream) {
    if (!ctx) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!stream) return COFHE_HIP_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    // An event keeps a pointer to the stream it was last recorded on, and the runtime looks at that stream (is it being
    // captured?) before it waits for the event: after hipStreamDestroy that is a read of freed memory, which came back as
    // hipErrorCapturedEvent / hipErrorStreamCaptureUnsupported from the hipEventSynchronize of cofhe_hip_malloc.  So nothing the
    // context keeps may still name this stream.  Its work has finished, so every event recorded on it has completed:
    // the workspace's last user, if it was this stream, leaves nothing to wait for (and a later stream that gets the same
    // handle value is not taken for it) ...
    if (ctx->ws_stream == (hipStream_t)stream) {
        ctx->ws_stream = nullptr;
        ctx->ws_event_set = false;
    }
    // ... and a cached block whose event has completed gets a fresh, unrecorded event, which any wait passes at once.  (An
    // event that has not completed was recorded on another stream, which is alive, and stays.)
    for (auto &kv : ctx->pool) {
        const hipError_t q = hipEventQuery(kv.second.ev);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            continue;
        }
        HIPCHK(q);
        hipEvent_t fresh = nullptr;
        HIPCHK(hipEventCreateWithFlags(&fresh, hipEventDisableTiming));
        (void)hipEventDestroy(kv.second.ev);
        kv.second.ev = fresh;
    }
    HIPCHK(hipStreamDestroy((hipStream_t)stream));
    return COFHE_HIP_OK;
}
int cofhe_hip_stream_query(cofhe_hip_ctx *ctx, void *stream, int *busy) {
    if (!ctx || !busy) return fail(COFHE_HIP_EINVAL, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    const hipError_t e = hipStreamQuery((hipStream_t)stream);
    if (e != hipSuccess && e != hipErrorNotReady) return fail(COFHE_HIP_EHIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
    if (e == hipErrorNotReady) (void)hipGetLastError();        // "not ready" is an answer: the thread's next checked launch must not see it
    *busy = e == hipErrorNotReady;
    return COFHE_HIP_OK;
}

int cofhe_hip_device_status(cofhe_hip_ctx *ctx, uint32_t *word, int clear, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!word) return fail(COFHE_HIP_EINVAL, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(word, ctx->d_status, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (clear) HIPCHK(hipMemsetAsync(ctx->d_status, 0, 4, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return COFHE_HIP_OK;
}

namespace {
// the checked launch of the launch helpers below, which this one entry precedes
extern "C++" template <typename... P, typename... A>
int launch(cofhe_hip_ctx *ctx, const char *span, void (*k)(P...), dim3 grid, dim3 block, hipStream_t st, A... args);
}  // namespace
int cofhe_hip_validate_records(cofhe_hip_ctx *ctx, const void *d_records, uint64_t n_records, int *all_valid, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!all_valid) return fail(COFHE_HIP_EINVAL, "null argument");
    *all_valid = 1;
    if (n_records == 0) return COFHE_HIP_OK;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned blocks;
    {
        const uint64_t b = (n_records + WG_GROUPS - 1) / WG_GROUPS;
        if (b > 0x7FFFFFFFull) return fail(COFHE_HIP_EINVAL, "work size out of range");
        blocks = (unsigned)b;
    }
    uint32_t *d_err = ctx->d_status + 1;              // second word of the status area: validation verdict
    HIPCHK(hipMemsetAsync(d_err, 0, 4, (hipStream_t)stream));
    if (int rc = launch(ctx, nullptr, k_validate_forms, blocks, WG_BLOCK, (hipStream_t)stream, (const uint32_t *)d_records, n_records,
                        (const uint32_t *)ctx->d_absdelta, d_err))
        return rc;
    uint32_t e = 0;
    HIPCHK(hipMemcpyAsync(&e, d_err, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    *all_valid = e == 0 ? 1 : 0;
    return COFHE_HIP_OK;
}

namespace {
constexpr size_t EXP_BYTES = (size_t)EXP_REC_WORDS * 4;       // one exponent record
constexpr size_t CT_BYTES = (size_t)2 * REC_WORDS * 4;        // one ciphertext: two form records
// The one range of k, 1 <= k <= 639, whichever bound a kernel names: 2 k + 1 bits fit one 1280-bit plane, the limbs of the
// plaintext kernels (PMM_MAX_LIMBS) and of the division (PDV_MAX_KBITS) hold k bits, and so does an exponent record
static_assert(PDV_MAX_KBITS == 32u * PMM_MAX_LIMBS - 1u && 2 * PDV_MAX_KBITS + 1 <= (uint32_t)PLIMBS * 32 &&
                  2 * (PDV_MAX_KBITS + 1) + 1 > (uint32_t)PLIMBS * 32 && PDV_MAX_KBITS <= EXP_MAG_WORDS * 32 - 1,
              "the bounds of k coincide");
constexpr bool k_in_range(uint64_t kbits) { return kbits >= 1 && kbits <= PDV_MAX_KBITS; }

// what an entry does once it has checked its arguments: its device made current, its stream as HIP's type
int on_device(cofhe_hip_ctx *ctx, void *stream, hipStream_t *st) {
    HIPCHK(hipSetDevice(ctx->device));
    *st = (hipStream_t)stream;
    return COFHE_HIP_OK;
}
// The overlap test of the entries: whether the output `out` is clear of every span of `others`.  An empty span overlaps nothing.
struct Span {
    const void *p;
    size_t bytes;
};
bool clear_of(Span out, std::initializer_list<Span> others) {
    const uintptr_t x = (uintptr_t)out.p;
    for (const Span &o : others) {
        const uintptr_t y = (uintptr_t)o.p;
        if (out.bytes && o.bytes && x < y + o.bytes && y < x + out.bytes) return false;
    }
    return true;
}
// whether every one of the pointers is 16-byte aligned (a caller's pointer is only known to be 4-byte aligned)
bool aligned16(std::initializer_list<const void *> ptrs) {
    uintptr_t all = 0;
    for (const void *p : ptrs) all |= (uintptr_t)p;
    return (all & 15) == 0;
}
// The grid of the kernels that move `records` records of `words` words in pieces: 16-byte pieces when the record length and
// the pointers of `ptrs` allow them, words otherwise; one thread per piece in workgroups of `threads`, 64 workgroups per CU at
// the most (the kernels stride beyond that)
struct PieceGrid {
    bool vec16;
    uint64_t total;              // pieces
    unsigned blocks;
    uint32_t flag() const { return vec16 ? 1u : 0u; }
};
PieceGrid piece_grid(uint64_t records, uint32_t words, unsigned threads, std::initializer_list<const void *> ptrs) {
    PieceGrid g;
    g.vec16 = words % 4 == 0 && aligned16(ptrs);
    g.total = records * (g.vec16 ? words / 4 : words);
    g.blocks = (unsigned)std::min<uint64_t>((g.total + threads - 1) / threads, 64u * NUM_CUS);
    return g;
}

struct DevBuf {                  // from the context's block cache
    cofhe_hip_ctx *ctx = nullptr;
    void *p = nullptr;
    void *stream;                // the block goes back behind the work queued on this stream (null: on any blocking stream)
    explicit DevBuf(void *s = nullptr) : stream(s) {}
    int get(cofhe_hip_ctx *c, size_t bytes) {
        ctx = c;
        return cofhe_hip_malloc(c, bytes, &p);
    }
    ~DevBuf() {
        if (p) (void)cofhe_hip_free_on_stream(ctx, p, stream);
    }
};
// RAII span of the "profile_kernels" option: two events on the launch stream around one kernel launch.  Spans are named after
// the kernel build actually launched, so that a test can tell which route a call took (cofhe_hip_profile_read's launch count)
struct ProfScope {
    cofhe_hip_ctx *ctx;
    hipStream_t st;
    cofhe_hip_ctx::ProfSpan sp{nullptr, nullptr, nullptr};
    ProfScope(cofhe_hip_ctx *c, const char *name, hipStream_t s) : ctx(c), st(s) {
        if (!c->opt_profile || !name || c->prof.size() >= 65536) return;
        if (hipEventCreate(&sp.a) != hipSuccess) return;
        if (hipEventCreate(&sp.b) != hipSuccess) {
            (void)hipEventDestroy(sp.a);
            return;
        }
        sp.name = name;
        (void)hipEventRecord(sp.a, st);
    }
    ~ProfScope() {
        if (!sp.name) return;
        (void)hipEventRecord(sp.b, st);
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);       // some launchers (compose, add) run without the context lock
        ctx->prof.push_back(sp);
    }
};
// The kernels with two builds (cofhe_hip.hip: k_compose_wg and k_compose_wg3, and their kin): the three-per-CU build (168
// registers per lane, fewer spills) whenever the whole grid is resident at three workgroups per CU, the plain build, which
// leaves room for four, otherwise
bool fits_three_per_cu(unsigned blocks) { return blocks <= 3u * NUM_CUS; }
// THE launch of a kernel with one build: in a "profile_kernels" span of the name `span` (null: none), and checked
extern "C++" template <typename... P, typename... A>
int launch(cofhe_hip_ctx *ctx, const char *span, void (*k)(P...), dim3 grid, dim3 block, hipStream_t st, A... args) {
    ProfScope ps(ctx, span, st);
    hipLaunchKernelGGL(k, grid, block, 0, st, args...);
    HIPCHK(hipGetLastError());
    return COFHE_HIP_OK;
}
// and of one with two: the build that fits a grid of `blocks` workgroups, in a span named span3 or span (null: none)
extern "C++" template <typename... P, typename... A>
int launch_wg(cofhe_hip_ctx *ctx, void (*k3)(P...), void (*k)(P...), const char *span3, const char *span, unsigned blocks,
              hipStream_t st, A... args) {
    return launch(ctx, fits_three_per_cu(blocks) ? span3 : span, fits_three_per_cu(blocks) ? k3 : k, blocks, WG_BLOCK, st, args...);
}
// What the four *_tuples_records entries do once they have checked their arguments: a block of the block cache for the `recs`
// plaintext rows, the rows by write_rows(block), and their fresh encryption into d_out, which carves the workspace by the plan
// "comb" (kind 1) over `recs` plaintexts
extern "C++" template <typename Rows>
int encrypt_rows(cofhe_hip_ctx *ctx, uint64_t recs, uint32_t kbits, const void *d_rho, const uint32_t *h_record, const uint32_t *pk_record,
                 const uint32_t *f_record, void *d_out, void *stream, Rows write_rows) {
    DevBuf rows(stream);
    if (int rc = rows.get(ctx, recs * EXP_BYTES)) return rc;
    if (int rc = write_rows(rows.p)) return rc;
    return cofhe_hip_encrypt_fresh_records(ctx, rows.p, d_rho, h_record, pk_record, f_record, d_out, recs, kbits, stream);
}
// The tail test of the four *_shape entries: whether shape_t is shape_e followed by `t` more dimensions, 8 at the most in all;
// *tail: those dimensions
bool tail_shape(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t t, const uint32_t **tail) {
    if (ndim_e > 8 - t || ndim_t != ndim_e + t || (ndim_e && memcmp(shape_t, shape_e, 4 * ndim_e) != 0)) return false;
    *tail = shape_t + ndim_e;
    return true;
}
int compose_blocks(uint64_t n, unsigned *blocks) {
    uint64_t b = (n + WG_GROUPS - 1) / WG_GROUPS;
    if (b == 0 || b > 0x7FFFFFFFull) return fail(COFHE_HIP_EINVAL, "work size out of range");
    *blocks = (unsigned)b;
    return COFHE_HIP_OK;
}
// one of the context's flag words for a one-word read-back or verdict of this call, handed out round robin (ctx.hpp) under
// the context lock, which the launchers that need nothing else of it (compose_wide, add) do not hold
uint32_t *flag_word(cofhe_hip_ctx *ctx) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return ctx->d_flags + (ctx->flag_next++ % cofhe_hip_ctx::N_FLAGS);
}
// grid of the k_c1_distinct / k_c1_spread scans over the records of n_ct ciphertexts
unsigned scan_blocks(uint64_t n_ct) { return (unsigned)std::min<uint64_t>((n_ct * REC_WORDS + 255) / 256, 2048); }
// the longest exponent of a call, which lives on the device: one small reduction and a 4-byte read-back
int max_exp_bits(cofhe_hip_ctx *ctx, const void *d_exps, uint64_t n_exps, hipStream_t st, uint32_t *bits) {
    uint32_t *d_bits = flag_word(ctx);
    HIPCHK(hipMemsetAsync(d_bits, 0, 4, st));
    if (int rc = launch(ctx, nullptr, k_exp_maxbits, (unsigned)((n_exps + 255) / 256), 256, st, (const uint32_t *)d_exps, n_exps, d_bits)) return rc;
    HIPCHK(hipMemcpyAsync(bits, d_bits, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return COFHE_HIP_OK;
}
// The lookup of the two table caches (ctx->fb and CombState::tabs; `dev` is the slot's device pointer): returns the filled slot
// that `match` accepts, or null, and in *victim the slot a miss may take: an empty one, else the least recently used, never
// one stamped by the current call (null when every slot is).  What happens on a miss is the caller's.
extern "C++" template <typename Slot, size_t N, typename Match>
Slot *cache_lookup(Slot (&slots)[N], uint32_t *Slot::*dev, uint64_t call_stamp, Match match, Slot **victim) {
    Slot *hit = nullptr;
    *victim = nullptr;
    for (Slot &s : slots) {
        if (s.*dev && match(s)) hit = &s;
        if (s.stamp == call_stamp) continue;                       // in use by this call
        if (!*victim || !(s.*dev) || ((*victim)->*dev && s.stamp < (*victim)->stamp)) *victim = &s;
    }
    return hit;
}

// ---- how the entry points carve the context's workspace ------------------------------------------------------------------
// Every launcher that uses the workspace takes its regions from ONE of the plan functions below, and
// cofhe_hip_workspace_plan hands the same plans out (host only, no GPU), so that a CPU test can check sizes and offsets --
// disjoint, ordered, each at least what its kernel indexes -- for any operand count without running anything.
extern "C++" {
struct WsPlan {
    static constexpr int MAX = 8;
    cofhe_hip_ws_region r[MAX];
    int n = 0;
    size_t total = 0;
    size_t add(const char *name, size_t bytes) {            // regions start on 256-byte boundaries
        const size_t off = (total + 255) & ~(size_t)255;
        if (n < MAX) {
            memset(&r[n], 0, sizeof(r[n]));
            strncpy(r[n].name, name, sizeof(r[n].name) - 1);
            r[n].offset = off;
            r[n].bytes = bytes;
            n++;
        }
        total = off + bytes;
        return off;
    }
    size_t off(const char *name) const {
        for (int i = 0; i < n; i++)
            if (strcmp(r[i].name, name) == 0) return (size_t)r[i].offset;
        return (size_t)-1;
    }
    size_t bytes(const char *name) const {
        for (int i = 0; i < n; i++)
            if (strcmp(r[i].name, name) == 0) return (size_t)r[i].bytes;
        return 0;
    }
};
constexpr uint32_t POW_SHARED_W = 6, POW_SHARED_TW = 1u << (POW_SHARED_W - 2);      // 16 odd powers per base: 10.5 KB
constexpr uint32_t POW_PAIR_MAX_LADDERS = 256;       // k_pow_shared_pair: two single-wavefront workgroups per ladder, all resident
// k_pow_shared over n_ladders bases: [front: the caller's records][table: (tw + 2) slots for every group of the GRID -- idle
// groups own slots too][digits of the one exponent][its length]
inline WsPlan plan_pow_shared(uint64_t n_ladders, size_t front_bytes) {
    WsPlan p;
    const uint64_t blocks = (n_ladders + WG_GROUPS - 1) / WG_GROUPS;
    p.add("front", front_bytes);
    p.add("table", (size_t)blocks * WG_GROUPS * (POW_SHARED_TW + 2) * REC_WORDS * 4);
    p.add("digits", (size_t)WNAF_POSITIONS);
    p.add("maxlen", 256);
    p.add("pairctl", (size_t)POW_PAIR_MAX_LADDERS * 16);       // k_pow_shared_pair: published / taken counts per ladder (zeroed with the digits)
    return p;
}
inline size_t accumulate_tree_bytes(uint32_t n, uint32_t m, uint32_t p) {
    return 2 * ((size_t)n * ((m + 1) / 2) * 2 * p * REC_WORDS * 4);
}
// the matrix product: [tables (tw > 1)][digits: WNAF_POSITIONS x m p bytes][maxlen][schedules: rcap words per column]
// [schedule lengths][partial products and their tree (segs > 1)]
inline uint32_t matmul_rcap(uint32_t exp_bits, uint32_t m, uint32_t segs) {
    const uint32_t seglen = (m + segs - 1) / segs;
    return (exp_bits + 2) * (seglen + 1) + 2;               // per position: a squaring and at most seglen products
}
inline WsPlan plan_scal_matmul(uint32_t n, uint32_t m, uint32_t p, uint32_t exp_bits, uint32_t w, uint32_t segs) {
    WsPlan q;
    const uint64_t nbase = (uint64_t)n * m * 2, n_exps = (uint64_t)m * p;
    const uint32_t tw = 1u << (w - 2);
    const uint32_t ncols = segs * p;
    q.add("table", tw > 1 ? (size_t)nbase * tw * REC_WORDS * 4 : 0);
    q.add("digits", (size_t)WNAF_POSITIONS * n_exps);
    q.add("maxlen", 256);
    q.add("ops", (size_t)ncols * matmul_rcap(exp_bits, m, segs) * 4);
    q.add("counts", (size_t)ncols * 4);
    q.add("partial", segs > 1 ? (size_t)n * segs * p * 2 * REC_WORDS * 4 : 0);
    q.add("tree", segs > 1 ? accumulate_tree_bytes(n, segs, p) : 0);
    return q;
}
// the product-tree form of the matrix product, what lives in the workspace: tables, digits, their length, and the per-level
// segment counts / offsets / totals of k_tree_plan (S_cap = (exp_bits + 2) p segments at most).  Entry lists, maps, the Horner
// schedule and the two level buffers are sized by the totals read back from `info` and come from the block cache.
// (nbase: the records the table is built over -- the n m 2 of the left operand, or the image of a convolution)
inline WsPlan plan_tree_over(uint64_t nbase, uint32_t m, uint32_t p, uint32_t exp_bits, uint32_t w) {
    WsPlan q;
    const uint64_t n_exps = (uint64_t)m * p;
    const uint32_t tw = 1u << (w - 2);
    const size_t S_cap = (size_t)(exp_bits + 2) * p;
    q.add("table", tw > 1 ? (size_t)nbase * tw * REC_WORDS * 4 : 0);
    q.add("digits", (size_t)WNAF_POSITIONS * n_exps);
    q.add("maxlen", 256);
    q.add("counts", (size_t)(TREE_LEVELS + 1) * S_cap * 4);
    q.add("offsets", (size_t)(TREE_LEVELS + 1) * (S_cap + 1) * 4);
    q.add("info", 256);
    return q;
}
inline WsPlan plan_scal_matmul_tree(uint32_t n, uint32_t m, uint32_t p, uint32_t exp_bits, uint32_t w) {
    return plan_tree_over((uint64_t)n * m * 2, m, p, exp_bits, w);
}
// the convolution's direct route: the tree's plan for m = kh kw C, p = Co, with the table over the B H W C 2 IMAGE records --
// every pixel once, not once per window it is in (no table at w = 2, as above: the image itself serves)
inline WsPlan plan_conv2d(const ConvShape &s, uint32_t exp_bits, uint32_t w) {
    return plan_tree_over((uint64_t)s.B * s.H * s.W * s.C * 2, conv_inner(s), s.Co, exp_bits, w);
}
inline WsPlan plan_accumulate_tree(uint32_t n, uint32_t m, uint32_t p) {
    WsPlan q;
    const size_t half = accumulate_tree_bytes(n, m, p) / 2;
    q.add("level_a", half);
    q.add("level_b", half);
    return q;
}
// one chunk of encrypt_tensor: [table pointers + slot counter][entry indices: cap x ne][level: cap x ne records]
// [next level: ceil(cap / 2) x ne records]
inline WsPlan plan_encrypt_chunk(uint64_t ne, uint32_t kbits) {
    WsPlan q;
    const uint32_t cap = kbits / 2 + 3;                      // pk^r + at most ceil((k + 1) / 2) digits
    q.add("header", 256);
    q.add("idx", (size_t)cap * ne * 4);
    q.add("level_a", (size_t)cap * ne * REC_WORDS * 4);
    q.add("level_b", ((size_t)(cap + 1) / 2) * ne * REC_WORDS * 4);
    return q;
}
// n fixed-base powers of at most mmax table entries each: two tree levels and the gather list (n pointers + n mmax indices)
inline WsPlan plan_fixed_base(uint32_t n, uint32_t mmax) {
    WsPlan q;
    const size_t half = (size_t)n * mmax * REC_WORDS * 4;
    q.add("level_a", half);
    q.add("level_b", half);
    q.add("gather", ((size_t)n + ((size_t)n * mmax + 1) / 2) * 8);
    return q;
}
// The fixed-base comb (comb.hpp): items are ciphertexts (kind 1 encrypt_fresh, 2 rerandomize: two columns each) or powers
// (kind 0: one column each); kind 3, the plaintext addend, has one column per ciphertext (its c2), kind 4, the addend with
// fresh randomness, an encryption's two columns and the leaf.  One chunk of `ne` items: [level_a: the fused first level, slots / 2 records per column]
// [level_b: the next level, ceil(slots / 4) per column]; the levels above alternate between the two.
constexpr uint64_t COMB_WS_LIMIT = 4ull << 30;               // one call's workspace, whatever n
constexpr uint64_t COMB_CHUNK_MAX = 65536;                   // items per pass when nothing else limits it
struct CombCall {
    CombShape s;
    uint32_t slots;
    uint64_t chunk;
};
inline CombShape comb_shape_of(uint32_t kind, uint32_t w, uint32_t exp_bits, uint32_t kbits) {
    CombShape s{};
    s.w = w;
    s.npos_r = kind == 3 ? 0u : comb_positions(exp_bits < COMB_EXP_BITS ? exp_bits : COMB_EXP_BITS, w);
    s.npos_m = kind == 1 || kind >= 3 ? comb_positions(kbits, w) : 0u;
    s.leaf = kind >= 2 ? 1u : 0u;
    s.halves = kind == 0 || kind == 3 ? 1u : 2u;
    s.kbits = kbits;
    s.c2_only = kind == 3 ? 1u : 0u;
    return s;
}
inline WsPlan plan_comb_chunk(const CombShape &s, uint64_t ne) {
    WsPlan q;
    const uint64_t cols = ne * s.halves, slots = comb_slots(s);
    q.add("level_a", (size_t)(slots / 2) * cols * REC_WORDS * 4);
    q.add("level_b", (size_t)((slots + 3) / 4) * cols * REC_WORDS * 4);
    return q;
}
// the launcher's decisions for n items whose longest exponent has exp_bits bits: w (pinned, or the widest, 10, for every
// count from 1 024 ciphertexts up -- fresh encryption of 16 384 took 62.6 / 45.5 / 36.3 ms at w = 6 / 8 / 10, 262 144: 1001 /
// 724 / 571 ms, profiles/r07_fresh; below that the call is latency and w does not matter; a table of 34 MB builds in 1.7 ms)
// and the chunk (pinned, or as many items as keep the workspace within COMB_WS_LIMIT)
inline uint32_t comb_auto_width(uint64_t n, uint32_t exp_bits) {
    (void)n;
    return exp_bits < 64 ? 4u : 10u;          // short exponents: a few positions at any w, and a table 64 times smaller
}
inline CombCall comb_call(uint32_t kind, uint64_t n, uint32_t exp_bits, uint32_t kbits, uint32_t w_pin, uint64_t chunk_pin) {
    CombCall c{};
    // kind 3 has no r: its one exponent is m mod 2^k, so k picks the width (and a context that also encrypts shares the table of f)
    c.s = comb_shape_of(kind, w_pin ? w_pin : comb_auto_width(n, kind == 3 ? kbits : exp_bits), exp_bits, kbits);
    c.slots = comb_slots(c.s);
    const uint64_t per_item = plan_comb_chunk(c.s, 1).total;
    uint64_t fit = (COMB_WS_LIMIT - 512) / per_item;
    if (fit > COMB_CHUNK_MAX) fit = COMB_CHUNK_MAX;
    c.chunk = chunk_pin ? (chunk_pin < fit ? chunk_pin : fit) : fit;
    if (n < c.chunk) c.chunk = n ? n : 1;
    return c;
}
}  // extern "C++"

// One user of the workspace at a time, on the device as well: the host lock (ctx->mu) only covers the enqueueing, the
// kernels run on after the entry point has returned.  A call on another stream first waits for the event the previous
// user recorded behind its last launch (calls on the same stream are ordered anyway); constructed under ctx->mu, before
// ensure_workspace, so that a reallocation's stream synchronisation covers the previous user too.
struct WsUse {
    cofhe_hip_ctx *ctx;
    hipStream_t st;
    WsUse(cofhe_hip_ctx *c, hipStream_t s) : ctx(c), st(s) {
        if (ctx->ws_event_set && ctx->ws_stream != st) (void)hipStreamWaitEvent(st, ctx->ws_event, 0);
    }
    ~WsUse() {
        if (!ctx->ws_event && hipEventCreateWithFlags(&ctx->ws_event, hipEventDisableTiming) != hipSuccess) {
            ctx->ws_event = nullptr;
            (void)hipStreamSynchronize(st);                    // no event to hand over: finish before anybody else starts
            ctx->ws_event_set = false;
            return;
        }
        ctx->ws_event_set = hipEventRecord(ctx->ws_event, st) == hipSuccess;
        ctx->ws_stream = st;
        if (!ctx->ws_event_set) (void)hipStreamSynchronize(st);
    }
};

// grow-only workspace of the context (tables, digit arrays, intermediate records)
int ensure_workspace(cofhe_hip_ctx *ctx, size_t need, hipStream_t st) {
    if (ctx->workspace_bytes >= need) return COFHE_HIP_OK;
    HIPCHK(hipStreamSynchronize(st));
    if (ctx->workspace) HIPCHK(hipFree(ctx->workspace));
    ctx->workspace = nullptr;
    ctx->workspace_bytes = 0;
    HIPCHK(dev_alloc(ctx, &ctx->workspace, need));
    ctx->workspace_bytes = need;
    return COFHE_HIP_OK;
}
}  // namespace

int cofhe_hip_compose_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n,
                              void *stream) {
    if (n == 0) return COFHE_HIP_OK;
    unsigned blocks;
    if (int rc = compose_blocks(n, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch_wg(ctx, k_compose_wg3, k_compose_wg, "k_compose_wg3", "k_compose_wg", blocks, st, (const uint32_t *)d_a,
                     (const uint32_t *)d_b, (uint32_t *)d_out, n, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
}

int cofhe_hip_compose_wide_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n, uint32_t reps,
                                   uint32_t *fallbacks, void *stream) {
    if (n == 0) return COFHE_HIP_OK;
    if (n > 0x7FFFFFFFull) return fail(COFHE_HIP_EINVAL, "work size out of range");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    uint32_t *d_fb = nullptr;
    if (fallbacks) {
        d_fb = flag_word(ctx);
        HIPCHK(hipMemsetAsync(d_fb, 0, 4, st));
    }
    if (int rc = launch(ctx, nullptr, k_compose_wide, (unsigned)n, 64, st, (const uint32_t *)d_a, (const uint32_t *)d_b, (uint32_t *)d_out, n,
                        reps, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status, d_fb))
        return rc;
    if (fallbacks) {
        HIPCHK(hipMemcpyAsync(fallbacks, d_fb, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return COFHE_HIP_OK;
}

namespace {
// the two builds of a ciphertext-pair kernel (k_add_ct / k_sub_ct and their three-per-CU forms) and their span names
using CtPairKernel = void (*)(const uint32_t *, const uint32_t *, uint32_t *, uint64_t, const uint32_t *, const uint32_t *, int, uint32_t *, uint32_t);
struct CtPairBuilds {
    CtPairKernel k3, k;
    const char *span3, *span;
};
// out[i] = a[i] (op) b[i] over n_ct ciphertexts: the c1 scan, the launch route that fits, the spread of a folded c1
int ct_pair_launch(cofhe_hip_ctx *ctx, const CtPairBuilds &kb, const void *d_a, const void *d_b, void *d_out, uint64_t n_ct, void *stream) {
    if (n_ct == 0) return COFHE_HIP_OK;
    if (n_ct > (1ull << 40)) return fail(COFHE_HIP_EINVAL, "tensor too large");
    unsigned blocks;
    if (int rc = compose_blocks(n_ct * 2, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    uint32_t *flag = flag_word(ctx);
    HIPCHK(hipMemsetAsync(flag, 0, 4, st));
    if (n_ct > 1) {
        if (int rc = launch(ctx, nullptr, k_c1_distinct, scan_blocks(n_ct), 256, st, (const uint32_t *)d_a, (const uint32_t *)d_b, n_ct, flag)) return rc;
    } else {
        HIPCHK(hipMemsetAsync(flag, 1, 1, st));                   // one ciphertext: nothing to fold
    }
    unsigned blocks_shared;
    if (int rc = compose_blocks(n_ct + 1, &blocks_shared)) return rc;
    const auto add = [&](unsigned grid, uint32_t only) {
        return launch_wg(ctx, kb.k3, kb.k, kb.span3, kb.span, grid, st, (const uint32_t *)d_a, (const uint32_t *)d_b, (uint32_t *)d_out,
                         n_ct, (const uint32_t *)flag, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status, only);
    };
    if (!fits_three_per_cu(blocks) && fits_three_per_cu(blocks_shared)) {
        // only the folded case fits at three per CU, and the host does not know which case it is: a pair of launches, each
        // sized and built for its case; the one whose case it is not returns at once (128x128: 0.308 -> 0.29x ms folded)
        if (int rc = add(blocks_shared, 1u)) return rc;
        if (int rc = add(blocks, 2u)) return rc;
    } else {
        if (int rc = add(blocks, 0u)) return rc;     // even with distinct c1, a grid that fits is resident at three workgroups per CU
    }
    if (n_ct > 1) return launch(ctx, nullptr, k_c1_spread, scan_blocks(n_ct), 256, st, (uint32_t *)d_out, n_ct, (const uint32_t *)flag);
    return COFHE_HIP_OK;
}
}  // namespace

int cofhe_hip_add_ciphertext_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n_ct, void *stream) {
    return ct_pair_launch(ctx, CtPairBuilds{k_add_ct3, k_add_ct, "k_add_ct3", "k_add_ct"}, d_a, d_b, d_out, n_ct, stream);
}
int cofhe_hip_sub_ciphertext_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n_ct, void *stream) {
    return ct_pair_launch(ctx, CtPairBuilds{k_sub_ct3, k_sub_ct, "k_sub_ct3", "k_sub_ct"}, d_a, d_b, d_out, n_ct, stream);
}

namespace {
// out[r] = in[r]^-1 for the records r = i stride + offset, i < n
int invert_launch(cofhe_hip_ctx *ctx, const void *d_in, void *d_out, uint64_t n, uint32_t stride, uint32_t offset, hipStream_t st) {
    unsigned blocks;
    if (int rc = compose_blocks(n, &blocks)) return rc;
    return launch(ctx, "k_invert_records", k_invert_records, blocks, WG_BLOCK, st, (const uint32_t *)d_in, (uint32_t *)d_out, n, stride, offset);
}
}  // namespace
int cofhe_hip_invert_records(cofhe_hip_ctx *ctx, const void *d_in, void *d_out, uint64_t n_records, void *stream) {
    if (n_records == 0) return COFHE_HIP_OK;
    if (!d_in || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return invert_launch(ctx, d_in, d_out, n_records, 1u, 0u, st);
}

namespace {
// k_pow keeps the running power in the output record: an output that overlaps the bases (in-place use) gets the bases
// copied to the workspace first
int pow_launch(cofhe_hip_ctx *ctx, const void *d_base, const void *d_exp, void *d_out, uint64_t n_records, uint32_t exp_mode, void *stream) {
    unsigned blocks;
    if (int rc = compose_blocks(n_records, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const size_t bytes = (size_t)n_records * REC_WORDS * 4;
    std::unique_lock<std::recursive_mutex> lk(ctx->mu, std::defer_lock);
    std::optional<WsUse> use;                                  // declared after the lock: released before it
    if (!clear_of({d_out, bytes}, {{d_base, bytes}})) {
        lk.lock();                                             // the workspace belongs to one call at a time ...
        use.emplace(ctx, st);                                  // ... until its kernel has finished (k_pow reads the copy)
        if (int rc = ensure_workspace(ctx, bytes, st)) return rc;
        HIPCHK(hipMemcpyAsync(ctx->workspace, d_base, bytes, hipMemcpyDeviceToDevice, st));
        d_base = ctx->workspace;
    }
    return launch(ctx, nullptr, k_pow, blocks, WG_BLOCK, st, (const uint32_t *)d_base, (const uint32_t *)d_exp, (uint32_t *)d_out, n_records,
                  1u, exp_mode, (const uint32_t *)ctx->d_one, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
}
// The pairwise product tree: folds src[n][mm][q] (mm slices of q records in each of n rows; a slice without a partner is
// paired with the principal form) down to one slice per row, ceil(log2 mm) k_compose_pairs launches.  The levels go to
// `next`, `other`, `next`, ... in turn -- the order is part of the caller's workspace plan, whose second buffer may only
// be large enough for the level after the first -- except the last one, which goes to `last` when that is given.  Each
// launch carries a span of the name `span` (null: none).  *result (if asked for): where the fold lies; src itself when mm == 1.
int product_tree(cofhe_hip_ctx *ctx, const uint32_t *src, uint32_t *next, uint32_t *other, uint32_t *last, uint32_t n, uint32_t mm, uint32_t q,
                 const char *span, hipStream_t st, const uint32_t **result) {
    while (mm > 1) {
        const uint32_t mh = (mm + 1) / 2;
        unsigned blocks;
        if (int rc = compose_blocks((uint64_t)n * mh * q, &blocks)) return rc;
        uint32_t *dst = mh == 1 && last ? last : next;
        if (int rc = launch(ctx, span, k_compose_pairs, blocks, WG_BLOCK, st, src, (const uint32_t *)ctx->d_one, dst, n, mm, q, 0u,
                            (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
            return rc;
        src = dst;
        std::swap(next, other);
        mm = mh;
    }
    if (result) *result = src;
    return COFHE_HIP_OK;
}
// tree_scratch: accumulate_tree_bytes() of device memory for the tree path, or nullptr to take it from the
// context workspace
int accumulate_impl(cofhe_hip_ctx *ctx, const void *d_x, const void *d_zero, void *d_out, uint32_t n, uint32_t m,
                    uint32_t p, void *tree_scratch, void *stream) {
    const uint64_t total = (uint64_t)n * p * 2;
    if (total == 0) return COFHE_HIP_OK;
    unsigned blocks;
    if (int rc = compose_blocks(total, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    if (total < 16384 && m >= 4) {
        // too few outputs to fill 256 CUs with chains of m compositions: pairwise product tree, ceil(log2 m)
        // launches over [n][m'][2p] slices in two ping-pong buffers, then the composition with Enc(0)
        const uint32_t q = 2 * p;
        const WsPlan tp = plan_accumulate_tree(n, m, p);
        if (!tree_scratch) {
            if (int rc = ensure_workspace(ctx, tp.total, st)) return rc;
            tree_scratch = ctx->workspace;
        }
        const uint32_t *src;
        if (int rc = product_tree(ctx, (const uint32_t *)d_x, (uint32_t *)((uint8_t *)tree_scratch + tp.off("level_a")),
                                  (uint32_t *)((uint8_t *)tree_scratch + tp.off("level_b")), nullptr, n, m, q, nullptr, st, &src))
            return rc;
        return launch(ctx, nullptr, k_compose_pairs, blocks, WG_BLOCK, st, src, (const uint32_t *)d_zero, (uint32_t *)d_out, n, 1u, q, 1u,
                      (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
    }
    return launch(ctx, nullptr, k_accumulate, blocks, WG_BLOCK, st, (const uint32_t *)d_x, (const uint32_t *)d_zero, (uint32_t *)d_out, n, m, p,
                  (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
}
}  // namespace

int cofhe_hip_pow_records(cofhe_hip_ctx *ctx, const void *d_base, const void *d_exp, void *d_out, uint64_t n_ct,
                          void *stream) {
    if (n_ct == 0) return COFHE_HIP_OK;
    return pow_launch(ctx, d_base, d_exp, d_out, n_ct * 2, 0u, stream);
}

int cofhe_hip_accumulate_records(cofhe_hip_ctx *ctx, const void *d_x, const void *d_zero, void *d_out, uint32_t n,
                                 uint32_t m, uint32_t p, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WsUse use(ctx, (hipStream_t)stream);
    return accumulate_impl(ctx, d_x, d_zero, d_out, n, m, p, nullptr, stream);
}

namespace {
// The chain base^(2^j), j < FIXED_BASE_CHAIN_LEN, of a base from the context's cache, built on a miss into the least recently
// used slot that this call (call_stamp) does not hold: one chain of ~1000 squarings on `st`.  The fixed-base powers and the
// comb tables (which start from every w-th entry) share it.
constexpr uint32_t FIXED_BASE_CHAIN_LEN = EXP_MAG_WORDS * 32 + 2;
int fixed_base_chain(cofhe_hip_ctx *ctx, const uint32_t *base_record, uint64_t call_stamp, hipStream_t st, cofhe_hip_ctx::FixedBase **out) {
    const uint32_t TABLE_LEN = FIXED_BASE_CHAIN_LEN;
    cofhe_hip_ctx::FixedBase *victim;
    cofhe_hip_ctx::FixedBase *fb = cache_lookup(ctx->fb, &cofhe_hip_ctx::FixedBase::d_table, call_stamp,
                                                [&](const cofhe_hip_ctx::FixedBase &e) { return memcmp(e.base, base_record, REC_WORDS * 4) == 0; }, &victim);
    if (!fb) {
        fb = victim;
        HIPCHK(hipStreamSynchronize(st));
        if (!fb->d_table) HIPCHK(dev_alloc(ctx, (void **)&fb->d_table, (size_t)(TABLE_LEN + 1) * REC_WORDS * 4));
        fb->len = 0;
        HIPCHK(hipMemcpyAsync(fb->d_table + (size_t)TABLE_LEN * REC_WORDS, base_record, REC_WORDS * 4, hipMemcpyHostToDevice, st));
        // one chain of ~1000 squarings: the latency kernel (one wavefront, wide layout); ladder_form 3 keeps the old one
        const bool old = ctx->opt_ladder_form == 3;
        if (int rc = launch(ctx, nullptr, old ? k_square_chain : k_square_chain_wide, 1, old ? WG_BLOCK : 64, st,
                            (const uint32_t *)(fb->d_table + (size_t)TABLE_LEN * REC_WORDS), fb->d_table, TABLE_LEN,
                            (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
            return rc;
        memcpy(fb->base, base_record, REC_WORDS * 4);
        fb->len = TABLE_LEN;
    }
    fb->stamp = call_stamp;
    *out = fb;
    return COFHE_HIP_OK;
}
}  // namespace

// out = base^e through the table base^(2^j) of the context (built by a chain of squarings on first use, then cached):
// the signed binary digits of e select ~bits/3 entries, which a pairwise product tree multiplies in ~log2 launches
// of a few hundred independent compositions -- milliseconds instead of the ~0.45 s serial ladder.  For the powers
// that always have the same base: h^r and pk^r of encryption (cpu_cryptosystem_tensor_ops.inl:7-12), h^sk of key generation.
int cofhe_hip_pow_fixed_base_records(cofhe_hip_ctx *ctx, uint32_t n, const uint32_t *base_records, const uint32_t *exp_records, void *d_out,
                                     void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!base_records || !exp_records || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (n == 0) return COFHE_HIP_OK;
    if (n > 4) return fail(COFHE_HIP_EINVAL, "at most 4 fixed-base powers per call (the context keeps 4 tables)");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    WsUse use(ctx, st);
    const uint32_t TABLE_LEN = FIXED_BASE_CHAIN_LEN;
    // ---- tables of the bases (all n must be resident at once: the ones of this call are stamped first)
    cofhe_hip_ctx::FixedBase *fbs[4] = {nullptr, nullptr, nullptr, nullptr};
    const uint64_t call_stamp = ++ctx->fb_clock;
    for (uint32_t b = 0; b < n; b++)
        if (int rc = fixed_base_chain(ctx, base_records + (size_t)b * REC_WORDS, call_stamp, st, &fbs[b])) return rc;
    // ---- non-adjacent form of |e| on the host: digit_i = bit_(i+1)(3x) - bit_(i+1)(x)
    std::vector<std::vector<uint32_t>> sel(n);
    uint32_t mmax = 1;
    for (uint32_t b = 0; b < n; b++) {
        const uint32_t *exp_record = exp_records + (size_t)b * EXP_REC_WORDS;
        const bool neg = exp_record[EXP_MAG_WORDS] != 0;
        uint32_t x3[EXP_MAG_WORDS + 1];
        uint64_t carry = 0;
        for (int w = 0; w < EXP_MAG_WORDS; w++) {
            const uint64_t t = (uint64_t)exp_record[w] * 3u + carry;
            x3[w] = (uint32_t)t;
            carry = t >> 32;
        }
        x3[EXP_MAG_WORDS] = (uint32_t)carry;
        auto bit = [](const uint32_t *v, int words, int i) -> int { return (i >> 5) < words ? (int)((v[i >> 5] >> (i & 31)) & 1u) : 0; };
        for (int i = 0; i < (int)TABLE_LEN; i++) {
            const int dgt = bit(x3, EXP_MAG_WORDS + 1, i + 1) - bit(exp_record, EXP_MAG_WORDS, i + 1);
            if (dgt != 0) sel[b].push_back((uint32_t)i | (b << 24) | (((dgt < 0) != neg) ? 0x80000000u : 0u));
        }
        if (sel[b].size() > mmax) mmax = (uint32_t)sel[b].size();
    }
    // ---- one gather and one product tree for all n powers (slices padded with the principal form)
    std::vector<uint64_t> host((size_t)n + ((size_t)n * mmax + 1) / 2);
    for (uint32_t b = 0; b < n; b++) host[b] = (uint64_t)(uintptr_t)fbs[b]->d_table;
    uint32_t *hidx = (uint32_t *)(host.data() + n);
    for (uint32_t b = 0; b < n; b++)
        for (uint32_t i = 0; i < mmax; i++) hidx[(size_t)b * mmax + i] = i < sel[b].size() ? sel[b][i] : 0xFFFFFFFFu;
    const WsPlan fp = plan_fixed_base(n, mmax);
    if (int rc = ensure_workspace(ctx, fp.total, st)) return rc;
    uint8_t *ws = (uint8_t *)ctx->workspace;
    uint64_t *d_tabs = (uint64_t *)(ws + fp.off("gather"));
    HIPCHK(hipMemcpyAsync(d_tabs, host.data(), host.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));          // `host` is a local vector: the copy must have read it before it goes
    uint32_t *buf[2] = {(uint32_t *)(ws + fp.off("level_a")), (uint32_t *)(ws + fp.off("level_b"))};
    const uint32_t total = n * mmax;
    if (int rc = launch(ctx, nullptr, k_gather_signed, (total + WG_GROUPS - 1) / WG_GROUPS, WG_BLOCK, st, (const uint64_t *)d_tabs,
                        (const uint32_t *)(d_tabs + n), (uint64_t)total, (const uint32_t *)ctx->d_one, buf[0]))
        return rc;
    const uint32_t *res;
    if (int rc = product_tree(ctx, buf[0], buf[1], buf[0], (uint32_t *)d_out, n, mmax, 1u, nullptr, st, &res)) return rc;
    if (res != d_out) HIPCHK(hipMemcpyAsync(d_out, res, (size_t)n * REC_WORDS * 4, hipMemcpyDeviceToDevice, st));     // mmax == 1: nothing to fold
    return COFHE_HIP_OK;
}
int cofhe_hip_pow_fixed_base_record(cofhe_hip_ctx *ctx, const uint32_t *base_record, const uint32_t *exp_record, void *d_out, void *stream) {
    return cofhe_hip_pow_fixed_base_records(ctx, 1, base_record, exp_record, d_out, stream);
}

int cofhe_hip_pow_form_records(cofhe_hip_ctx *ctx, const void *d_base, const void *d_exp, void *d_out, uint64_t n_forms,
                               void *stream) {
    if (n_forms == 0) return COFHE_HIP_OK;
    return pow_launch(ctx, d_base, d_exp, d_out, n_forms, 1u, stream);
}

// ---- the fixed-base comb (comb.hpp, comb.hip) -----------------------------------------------------------------------------
// base^e[i] for many exponents against one cached table per (base, w): one fused gather + first-level launch and the
// k_compose_pairs levels of a pairwise tree per chunk, ~floor(bits/w) + 1 compositions per power and no squarings.
namespace {
int comb_check(uint64_t kind, uint64_t n, uint64_t exp_bits, uint64_t kbits, uint64_t w, uint64_t chunk) {
    if (kind > 4)
        return fail(COFHE_HIP_EINVAL, "comb: kind 0 (powers), 1 (fresh encryption), 2 (re-randomisation), 3 (plaintext addend) or 4 (addend with randomness)");
    if (n > (1ull << 36)) return fail(COFHE_HIP_EINVAL, "comb: too many items");
    if (exp_bits > COMB_EXP_BITS) return fail(COFHE_HIP_EINVAL, "comb: exponents have at most 992 bits");
    if (w != 0 && (w < (uint64_t)COMB_W_MIN || w > (uint64_t)COMB_W_MAX)) return fail(COFHE_HIP_EINVAL, "comb: w is 0 (automatic) or 2..10");
    if ((kind == 1 || kind >= 3) && !k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (chunk > (1ull << 32)) return fail(COFHE_HIP_EINVAL, "comb: chunk out of range");
    return COFHE_HIP_OK;
}

// the comb table of (base, w), from the cache or built on `st`: T[j][1] = chain entry w j (one strided copy), then the
// w - 1 levels of k_comb_table.  The tables of one call are all stamped with call_stamp and are not evicted by it.
int comb_table(cofhe_hip_ctx *ctx, const uint32_t *base_record, uint32_t w, uint64_t call_stamp, hipStream_t st, const uint32_t **out) {
    CombState &cs = comb_state(ctx);
    CombTable *victim;
    CombTable *hit = cache_lookup(cs.tabs, &CombTable::d, call_stamp,
                                  [&](const CombTable &t) { return t.w == w && memcmp(t.base, base_record, REC_WORDS * 4) == 0; }, &victim);
    if (!hit) {
        if (!victim) return fail(COFHE_HIP_EINVAL, "comb: no table slot left");
        hit = victim;
        const uint32_t npos = comb_table_positions(w), D = comb_entries(w);
        HIPCHK(hipStreamSynchronize(st));                         // the slot's previous table may still be read
        if (hit->d) HIPCHK(hipFree(hit->d));
        hit->d = nullptr;
        hit->w = 0;
        HIPCHK(dev_alloc(ctx, (void **)&hit->d, (size_t)npos * D * REC_WORDS * 4));
        cofhe_hip_ctx::FixedBase *fb = nullptr;
        if (int rc = fixed_base_chain(ctx, base_record, ++ctx->fb_clock, st, &fb)) return rc;
        HIPCHK(hipMemcpy2DAsync(hit->d, (size_t)D * REC_WORDS * 4, fb->d_table, (size_t)w * REC_WORDS * 4, REC_WORDS * 4, npos,
                                hipMemcpyDeviceToDevice, st));
        for (uint32_t half = 1; half < D; half *= 2) {
            unsigned blocks;
            if (int rc = compose_blocks((uint64_t)npos * half, &blocks)) return rc;
            if (int rc = launch(ctx, "k_comb_table", k_comb_table, blocks, WG_BLOCK, st, hit->d, npos, w, half, (const uint32_t *)ctx->d_absdelta,
                                ctx->half_dbits, ctx->d_status))
                return rc;
        }
        memcpy(hit->base, base_record, REC_WORDS * 4);
        hit->w = w;
    }
    hit->stamp = call_stamp;
    *out = hit->d;
    return COFHE_HIP_OK;
}

// kind 0: out[i] = base0^r[i] (n records); 1: out[2i] = h^r[i], out[2i+1] = pk^r[i] o f^(m[i] mod 2^k); 2: out[2i] =
// leaf[2i] o h^r[i], out[2i+1] = leaf[2i+1] o pk^r[i]; 3: out[2i+1] = leaf[2i+1] o f^m[i], the records 2i copied (d_out
// other than d_leaf) -- no r, no read-back; 4: out[2i] = leaf[2i] o h^r[i], out[2i+1] = leaf[2i+1] o pk^r[i] o f^m[i].
// mode (kinds 3, 4): 0 as written, 1 m negated (ct - m), 2 every leaf inverted (m - ct; kind 3 inverts the records 2i too).
// bases: host records of (base0 | h, pk, f) as the kind needs.
int comb_run(cofhe_hip_ctx *ctx, uint32_t kind, const uint32_t *const bases[3], const void *d_r, const void *d_m, const void *d_leaf,
             void *d_out, uint64_t n, uint32_t kbits, void *stream, int mode = 0) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    static const unsigned NEEDS[5] = {1u, 7u, 3u, 4u, 7u};       // which of (base0 | h, pk, f) a kind reads
    if (kind > 4) return fail(COFHE_HIP_EINVAL, "comb: no such kind");
    for (int b = 0; b < 3; b++)
        if ((NEEDS[kind] >> b & 1u) && !bases[b]) return fail(COFHE_HIP_EINVAL, "null argument");
    if (int rc = comb_check(kind, n, 0, kbits, 0, 0)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    const bool has_r = kind != 3, has_m = kind == 1 || kind >= 3, has_leaf = kind >= 2;
    if (!d_out || (has_r && !d_r) || (has_m && !d_m) || (has_leaf && !d_leaf)) return fail(COFHE_HIP_EINVAL, "null argument");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    WsUse use(ctx, st);
    const CombState &cs = comb_state(ctx);
    // the tree's shape follows the longest exponent: the one read-back of the call (kind 3: its shape follows from k alone)
    uint32_t exp_bits = 0;
    if (has_r)
        if (int rc = max_exp_bits(ctx, d_r, n, st, &exp_bits)) return rc;
    CombCall cc = comb_call(kind, n, exp_bits, kbits, cs.opt_width, cs.opt_chunk);
    cc.s.m_neg = mode == 1 ? 1u : 0u;
    cc.s.leaf_inv = mode == 2 ? 1u : 0u;
    const uint64_t call_stamp = ++comb_state(ctx).clock;
    const uint32_t *tabs[3] = {nullptr, nullptr, nullptr};
    for (int b = 0; b < 3; b++)
        if (NEEDS[kind] >> b & 1u)
            if (int rc = comb_table(ctx, bases[b], cc.s.w, call_stamp, st, &tabs[b])) return rc;
    const WsPlan wp = plan_comb_chunk(cc.s, cc.chunk);
    if (int rc = ensure_workspace(ctx, wp.total, st)) return rc;
    uint8_t *ws = (uint8_t *)ctx->workspace;
    uint32_t *buf[2] = {(uint32_t *)(ws + wp.off("level_a")), (uint32_t *)(ws + wp.off("level_b"))};
    // R: records per item in the caller's tensors (kind 3 has one column, the second record of a ciphertext)
    const uint32_t H = cc.s.halves, R = kind == 3 ? 2u : H;
    const size_t rec_bytes = (size_t)REC_WORDS * 4;
    if (kind == 3) {                 // the c1 records: inverted (m - ct), copied, or left where they are
        if (mode == 2) {
            if (int rc = invert_launch(ctx, d_leaf, d_out, n, 2u, 0u, st)) return rc;
        } else if (d_out != d_leaf) {
            HIPCHK(hipMemcpy2DAsync(d_out, 2 * rec_bytes, d_leaf, 2 * rec_bytes, rec_bytes, n, hipMemcpyDeviceToDevice, st));
        }
    }
    for (uint64_t e0 = 0; e0 < n; e0 += cc.chunk) {
        const uint64_t ne = n - e0 < cc.chunk ? n - e0 : cc.chunk, ncols = ne * H;
        uint32_t *out = (uint32_t *)d_out + e0 * R * REC_WORDS;
        uint32_t mm = cc.slots / 2;
        unsigned blocks;
        if (int rc = compose_blocks(ncols * mm, &blocks)) return rc;
        if (int rc = launch(ctx, "k_comb_first", k_comb_first, blocks, WG_BLOCK, st, cc.s, tabs[0], tabs[1], tabs[2],
                            d_r ? (const uint32_t *)d_r + e0 * EXP_REC_WORDS : nullptr, d_m ? (const uint32_t *)d_m + e0 * EXP_REC_WORDS : nullptr,
                            d_leaf ? (const uint32_t *)d_leaf + e0 * R * REC_WORDS : nullptr, ncols, (const uint32_t *)ctx->d_one,
                            mm == 1 && kind != 3 ? out : buf[0], (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
            return rc;
        // kind 3's columns are every second record of the output: its tree ends in the workspace and one strided copy places it
        const uint32_t *top = nullptr;
        if (int rc = product_tree(ctx, buf[0], buf[1], buf[0], kind == 3 ? nullptr : out, 1u, mm, (uint32_t)ncols, "k_compose_pairs", st, &top))
            return rc;
        if (kind == 3) HIPCHK(hipMemcpy2DAsync(out + REC_WORDS, 2 * rec_bytes, top, rec_bytes, rec_bytes, ne, hipMemcpyDeviceToDevice, st));
    }
    return COFHE_HIP_OK;
}
}  // namespace

int cofhe_hip_pow_fixed_base_many_records(cofhe_hip_ctx *ctx, const uint32_t *base_record, const void *d_exps, void *d_out, uint64_t n,
                                          void *stream) {
    const uint32_t *bases[3] = {base_record, nullptr, nullptr};
    return comb_run(ctx, 0, bases, d_exps, nullptr, nullptr, d_out, n, 0, stream);
}
int cofhe_hip_encrypt_fresh_records(cofhe_hip_ctx *ctx, const void *d_plain, const void *d_r, const uint32_t *h_record, const uint32_t *pk_record,
                                    const uint32_t *f_record, void *d_out, uint64_t n_ct, uint32_t kbits, void *stream) {
    const uint32_t *bases[3] = {h_record, pk_record, f_record};
    return comb_run(ctx, 1, bases, d_r, d_plain, nullptr, d_out, n_ct, kbits, stream);
}
int cofhe_hip_rerandomize_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_r, const uint32_t *h_record, const uint32_t *pk_record,
                                  void *d_out, uint64_t n_ct, void *stream) {
    const uint32_t *bases[3] = {h_record, pk_record, nullptr};
    return comb_run(ctx, 2, bases, d_r, nullptr, d_cts, d_out, n_ct, 0, stream);
}
int cofhe_hip_add_plain_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_plain, const void *d_r, const uint32_t *h_record,
                                const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n_ct, uint32_t kbits, int mode,
                                void *stream) {
    if (mode < 0 || mode > 2) return fail(COFHE_HIP_EINVAL, "add_plain: mode 0 (ct + m), 1 (ct - m) or 2 (m - ct)");
    const uint32_t *bases[3] = {d_r ? h_record : nullptr, d_r ? pk_record : nullptr, f_record};
    return comb_run(ctx, d_r ? 4u : 3u, bases, d_r, d_plain, d_cts, d_out, n_ct, kbits, stream, mode);
}
int cofhe_hip_comb_shape(uint32_t kind, uint64_t n, uint32_t exp_bits, uint32_t kbits, uint32_t w_pin, uint64_t chunk_pin, uint32_t *w,
                         uint32_t *slots, uint64_t *chunk) {
    if (!w || !slots || !chunk) return fail(COFHE_HIP_EINVAL, "null argument");
    if (int rc = comb_check(kind, n, exp_bits, kbits, w_pin, chunk_pin)) return rc;
    const CombCall cc = comb_call(kind, n, exp_bits, kbits, w_pin, chunk_pin);
    *w = cc.s.w;
    *slots = cc.slots;
    *chunk = cc.chunk;
    return COFHE_HIP_OK;
}

namespace {
// out[i] = base[i * stride]^e, e one exponent record on the device; extra_bytes of the workspace are
// left free in front for the caller (returned through *extra)
int pow_shared(cofhe_hip_ctx *ctx, const void *d_base, uint32_t stride, const void *d_exp, void *d_out, uint64_t n,
               size_t extra_bytes, void **extra, hipStream_t st) {
    unsigned blocks;
    if (int rc = compose_blocks(n, &blocks)) return rc;
    const uint32_t w = POW_SHARED_W, tw = POW_SHARED_TW;
    const WsPlan pp = plan_pow_shared(n, extra_bytes);         // front | table: odd powers, x^2, running power | digits | length
    if (int rc = ensure_workspace(ctx, pp.total, st)) return rc;
    uint8_t *ws = (uint8_t *)ctx->workspace;
    if (extra) *extra = ws + pp.off("front");
    if (!d_out) d_out = ws + pp.off("front");                  // result into the caller's part of the workspace
    uint32_t *table = (uint32_t *)(ws + pp.off("table"));
    int8_t *digits = (int8_t *)(ws + pp.off("digits"));
    uint32_t *maxlen = (uint32_t *)(ws + pp.off("maxlen"));
    uint32_t *pairctl = (uint32_t *)(ws + pp.off("pairctl"));
    HIPCHK(hipMemsetAsync(digits, 0, pp.off("pairctl") + (size_t)POW_PAIR_MAX_LADDERS * 16 - pp.off("digits"), st));
    // Few ladders (one, when a tensor shares its c1): latency is all there is -- the wavefront-wide layout (wide.hip), a pair
    // of wavefronts per ladder (one squares, one multiplies: k_pow_shared_pair, non-adjacent digits), up to one ladder per CU
    // (profiles/r04_a/wide_time.txt); "ladder_form" pins the choice (1: the pair, 2: the 8-lane solo form of round 4's first
    // step, 3: the throughput kernel, 4: one wavefront per ladder, left to right with a table of odd powers)
    int form = ctx->opt_ladder_form ? ctx->opt_ladder_form : (n <= 256 ? 1 : 3);           // one ladder per CU at most: four per CU ran at half speed each
    if (form == 1 && n > POW_PAIR_MAX_LADDERS) form = 4;        // the pair's two workgroups must be resident together
    if (int rc = launch(ctx, nullptr, k_wnaf_digits, 1, 64, st, (const uint32_t *)d_exp, (uint64_t)1, form == 1 ? 2u : w, digits, maxlen)) return rc;
    // forms 4, 2 (while its ladders fit one wavefront) and 3 take the same arguments; the span is named after the kernel
    struct Ladder {
        decltype(&k_pow_shared) kernel;
        unsigned grid, block;
        const char *span;
    };
    const Ladder l = form == 4                    ? Ladder{k_pow_shared_wide, (unsigned)n, 64, "k_pow_shared_wide"}
                     : (form == 2 && n <= 64 / G) ? Ladder{k_pow_shared_solo, 1, 64, "k_pow_shared_solo"}
                                                  : Ladder{k_pow_shared, blocks, WG_BLOCK, "k_pow_shared"};
    if (form == 1)
        return launch(ctx, "k_pow_shared_pair", k_pow_shared_pair, (unsigned)(2 * n), 64, st, (const uint32_t *)d_base, (const int8_t *)digits,
                      (const uint32_t *)maxlen, table, pairctl, (uint32_t *)d_out, n, stride, (const uint32_t *)ctx->d_one,
                      (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);     // the table region serves as the rings
    return launch(ctx, l.span, l.kernel, l.grid, l.block, st, (const uint32_t *)d_base, (const int8_t *)digits, (const uint32_t *)maxlen, table,
                  (uint32_t *)d_out, n, stride, tw, (const uint32_t *)ctx->d_one, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits,
                  ctx->d_status);
}
// out[i] = c1_i^e for the n_ct ciphertexts of a tensor (decryption, threshold decryption).  A tensor that encrypt_tensor
// made -- or a sum of such tensors -- carries ONE c1 (cpu_cryptosystem_tensor_ops.inl:7-12): then one ladder runs and its
// result is copied, instead of n_ct identical ladders of ~1100 compositions each (the latency of the call stays that
// of one ladder; what goes away is the work: a 1024x1024 tensor decrypts ~8x faster).  Found out per call by one
// pass over the c1 records; tensors with differing c1 (results of scal_ciphertext_tensors) take the plain path.
int pow_shared_c1(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_exp, void *d_out, uint64_t n_ct, size_t extra_bytes, void **extra,
                  hipStream_t st) {
    bool shared = false;
    if (n_ct >= 64) {
        uint32_t *flag = flag_word(ctx);
        HIPCHK(hipMemsetAsync(flag, 0, 4, st));
        if (int rc = launch(ctx, nullptr, k_c1_distinct, scan_blocks(n_ct), 256, st, (const uint32_t *)d_cts, (const uint32_t *)d_cts, n_ct, flag)) return rc;
        uint32_t distinct = 1;
        HIPCHK(hipMemcpyAsync(&distinct, flag, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        shared = distinct == 0;
    }
    if (!shared) return pow_shared(ctx, d_cts, 2, d_exp, d_out, n_ct, extra_bytes, extra, st);
    void *ex = nullptr;
    if (int rc = pow_shared(ctx, d_cts, 2, d_exp, d_out, 1, extra_bytes, &ex, st)) return rc;
    if (extra) *extra = ex;
    uint32_t *res = (uint32_t *)(d_out ? d_out : ex);
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_ct * REC_WORDS + 255) / 256, 4096);
    return launch(ctx, "k_spread_records", k_spread_records, blocks, 256, st, res, n_ct);     // the witness of the shared route: one ladder, then this copy
}
}  // namespace

int cofhe_hip_part_decrypt_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_share, void *d_out,
                                   uint64_t n_ct, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_ct == 0) return COFHE_HIP_OK;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    WsUse use(ctx, st);
    return pow_shared_c1(ctx, d_cts, d_share, d_out, n_ct, 0, nullptr, st);
}

namespace {
// ---- the matrix product: what its two routes share, the routes, then the entry point that chooses ------------------------
// the width-w digits of n_exps exponents and the length of the longest, in a "k_wnaf_digits" span
int wnaf_digits(cofhe_hip_ctx *ctx, const void *d_exp, uint64_t n_exps, uint32_t w, int8_t *digits, uint32_t *maxlen, hipStream_t st) {
    if (n_exps == 0) return COFHE_HIP_OK;
    return launch(ctx, "k_wnaf_digits", k_wnaf_digits, (unsigned)((n_exps + 255) / 256), 256, st, (const uint32_t *)d_exp, n_exps, w, digits, maxlen);
}
// the tw odd powers of each of the nbase records into `room`, in a "k_pow_table" span (around the "k_pow_table3" one of the
// three-per-CU build); *table: where the route finds them
int pow_table(cofhe_hip_ctx *ctx, const void *d_cts, uint64_t nbase, uint32_t tw, void *room, hipStream_t st, const uint32_t **table) {
    *table = (const uint32_t *)d_cts;                         // w == 2: the only table entry is the base itself
    if (tw == 1 || nbase == 0) return COFHE_HIP_OK;
    unsigned tblocks;
    if (int rc = compose_blocks(nbase, &tblocks)) return rc;
    ProfScope ps(ctx, "k_pow_table", st);
    if (int rc = launch_wg(ctx, k_pow_table3, k_pow_table, "k_pow_table3", nullptr, tblocks, st, (const uint32_t *)d_cts, (uint32_t *)room, nbase, tw,
                           (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
        return rc;
    *table = (const uint32_t *)room;
    return COFHE_HIP_OK;
}

// The window width of a product whose table is built over nbase records, each of which `uses` output columns read: a table
// of 2^(w-2) odd powers per base costs that many compositions and saves ~bits (1/3 - 1/(w+1)) in each of its uses; the tables
// stay under 1/8 of the device memory.  "wnaf_width" pins the choice.
int wnaf_auto_width(cofhe_hip_ctx *ctx, uint64_t nbase, double uses, uint32_t exp_bits, uint32_t *width) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    uint32_t w = 2;
    double best = uses * exp_bits / 3.0;                           // w = 2: plain NAF, no table
    for (uint32_t cand = 3; cand <= 8; cand++) {
        const uint64_t bytes = nbase * (1ull << (cand - 2)) * REC_WORDS * 4;
        if (bytes > total_b / 8 || bytes > free_b / 2) break;
        const double cost = (double)(1u << (cand - 2)) + uses * exp_bits / (cand + 1.0);
        if (cost < best) {
            best = cost;
            w = cand;
        }
    }
    if (ctx->opt_wnaf_width >= 2 && ctx->opt_wnaf_width <= 8) w = ctx->opt_wnaf_width;      // cofhe_hip_ctx_set_option
    *width = w;
    return COFHE_HIP_OK;
}

// The product-tree route (k_tree_*) at window width w for exponents of at most exp_bits bits.  *taken = false: declined --
// only the digits and the plan have been computed, no output written -- and the caller runs the chains instead.
// cv (null for the matrix product): the product is a convolution -- d_cts is the image, the table is built over ITS records,
// and level 0 finds its leaves through conv_leaf (k_conv_level0); n = conv_rows, m = conv_inner, p = Co.  chunk_rows (a
// convolution's "conv_chunk_rows"): that many rows per chunk, whatever fits and without the rounding.
int matmul_tree_route(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_exp, const void *d_zero, void *d_out, uint32_t n, uint32_t m, uint32_t p,
                      uint32_t w, uint32_t exp_bits, hipStream_t st, bool *taken, const ConvShape *cv = nullptr, uint32_t chunk_rows = 0) {
    *taken = false;
    const uint64_t nbase = cv ? (uint64_t)cv->B * cv->H * cv->W * cv->C * 2 : (uint64_t)n * m * 2, n_exps = (uint64_t)m * p;
    const uint32_t tw = 1u << (w - 2);
    const WsPlan tp = cv ? plan_conv2d(*cv, exp_bits, w) : plan_scal_matmul_tree(n, m, p, exp_bits, w);
    if (int rc = ensure_workspace(ctx, tp.total, st)) return rc;
    uint8_t *ws = (uint8_t *)ctx->workspace;
    int8_t *digits = (int8_t *)(ws + tp.off("digits"));
    uint32_t *maxlen = (uint32_t *)(ws + tp.off("maxlen"));
    uint32_t *d_c = (uint32_t *)(ws + tp.off("counts")), *d_off = (uint32_t *)(ws + tp.off("offsets"));
    uint32_t *d_info = (uint32_t *)(ws + tp.off("info"));
    const uint32_t S_cap = (exp_bits + 2) * p;
    HIPCHK(hipMemsetAsync(digits, 0, tp.off("maxlen") + 256 - tp.off("digits"), st));
    if (int rc = wnaf_digits(ctx, d_exp, n_exps, w, digits, maxlen, st)) return rc;
    HIPCHK(hipMemsetAsync(d_c, 0, (size_t)S_cap * 4, st));              // level 0 of segments beyond the longest exponent
    if (int rc = launch(ctx, nullptr, k_tree_count, (unsigned)(((uint64_t)S_cap + 255) / 256), 256, st, (const int8_t *)digits,
                        (const uint32_t *)maxlen, m, p, d_c))
        return rc;
    if (int rc = launch(ctx, nullptr, k_tree_plan, 1, 1024, st, (const uint32_t *)maxlen, p, S_cap, d_c, d_off, d_info)) return rc;
    uint32_t info[TREE_LEVELS + 3];
    HIPCHK(hipMemcpyAsync(info, d_info, sizeof(info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                           // `info` is on the host
    const uint32_t T = info[TREE_LEVELS + 1], S = info[TREE_LEVELS + 2];
    if (T < 1 || T > TREE_LEVELS || S > S_cap) return fail(COFHE_HIP_EHIP, "matrix product: tree plan out of range");
    // rows per chunk: the two level buffers hold N_1 x rows x 2 records each (level 1 is the largest) ...
    const uint64_t n1 = info[1] ? info[1] : 1;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // ... and small enough for the context's block cache to keep both of them between calls (a quarter of its cap each):
    // buffers beyond the cap are given back to the driver at the end of every call, and allocating tens of GB anew
    // cost the product more than its kernels (bench.py, first tree build: 2.03 s per 256^3 product of which 0.78 s compute)
    const uint64_t budget = std::min<uint64_t>(free_b / 4, std::max<uint64_t>(ctx->pool_cap / 4, (uint64_t)1 << 30));
    uint64_t R = budget / (n1 * 2 * REC_WORDS * 4);
    if (R >= 16) R &= ~(uint64_t)15;                           // 2 R a multiple of 32: the groups of a workgroup share their element
    if (chunk_rows) R = chunk_rows;
    if (R < 1) R = 1;
    if (R > n) R = n;
    // Long exponents make long trees (N_1 ~ p bits m / 2 (w + 1) elements per row): when fewer than 16 rows fit a chunk the
    // workgroups mix tree elements, copies ride along as dummy compositions, and the chains win again (32x256.256x256 with
    // 128-bit exponents: 0.83 s in 14-row chunks against 0.68 s; profiles/r04_a/tree_time_chunks.txt)
    // The Horner chains address the top level's N_T elements through the op word's 21-bit base index (off_T[s] < N_T):
    // beyond 2^21 elements the tree is not taken, "matmul_tree" = 1 included, and the chains run instead
    const bool tree_fits = info[T] <= MM_INDEX_LIMIT;
    const bool tree_pays = tree_fits && (R >= 16 || R == n || ctx->opt_matmul_tree == 1 || chunk_rows);
    if (!tree_pays) return COFHE_HIP_OK;
    const uint32_t *table;
    if (int rc = pow_table(ctx, d_cts, nbase, tw, ws + tp.off("table"), st, &table)) return rc;
    uint64_t map_words = 0;
    for (uint32_t l = 1; l <= T; l++) map_words += info[l];
    const uint32_t len = p ? S / p : 0;                       // bit positions in use
    const uint32_t rcap_h = 2 * len + 2;
    DevBuf b_ent(st), b_map(st), b_ops(st), b_cnt(st), b_lvl[2] = {DevBuf(st), DevBuf(st)};      // back behind `st` on every way out
    if (int rc = b_ent.get(ctx, (size_t)info[0] * 4 + 4)) return rc;
    if (int rc = b_map.get(ctx, (size_t)map_words * 4 + 4)) return rc;
    if (int rc = b_ops.get(ctx, (size_t)p * rcap_h * 4)) return rc;
    if (int rc = b_cnt.get(ctx, (size_t)p * 4)) return rc;
    if (int rc = launch(ctx, nullptr, k_tree_fill, S ? S : 1, 64, st, (const int8_t *)digits, m, p, S_cap, (const uint32_t *)d_c,
                        (const uint32_t *)d_off, (const uint32_t *)d_info, (uint32_t *)b_ent.p, (uint32_t *)b_map.p))
        return rc;
    if (int rc = launch(ctx, nullptr, k_tree_horner_schedule, (p + 63) / 64, 64, st, (const uint32_t *)maxlen, p, S_cap, (const uint32_t *)d_c,
                        (const uint32_t *)d_off, (const uint32_t *)d_info, rcap_h, (uint32_t *)b_ops.p, (uint32_t *)b_cnt.p, ctx->d_status))
        return rc;
    const size_t lvl_bytes = (size_t)n1 * R * 2 * REC_WORDS * 4;
    if (int rc = b_lvl[0].get(ctx, lvl_bytes)) return rc;
    if (int rc = b_lvl[1].get(ctx, lvl_bytes)) return rc;
    const uint32_t *maps = (const uint32_t *)b_map.p;
    for (uint32_t r0 = 0; r0 < n; r0 += (uint32_t)R) {
        const uint32_t rows = std::min<uint32_t>((uint32_t)R, n - r0);
        uint64_t map_base = 0;
        for (uint32_t l = 0; l < T; l++) {                     // level l -> l + 1
            const uint64_t items = (uint64_t)info[l + 1] * rows * 2;
            unsigned lb;
            if (items == 0) break;
            if (int rc = compose_blocks(items, &lb)) return rc;
            if (cv && l == 0) {                                // the leaves of rows r0 .. r0 + rows - 1, from the image's table
                if (int rc = launch(ctx, "k_conv_level0", k_conv_level0, lb, WG_BLOCK, st, *cv, table, (const uint32_t *)ctx->d_one,
                                    (const uint32_t *)b_ent.p, (const uint32_t *)d_off, (const uint32_t *)(d_off + (S_cap + 1)), maps, info[1], r0, rows,
                                    tw, (uint32_t *)b_lvl[0].p, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
                    return rc;
                map_base += info[1];
                continue;
            }
            const uint32_t *src = l == 0 ? table + (uint64_t)r0 * m * 2 * tw * REC_WORDS : (const uint32_t *)b_lvl[(l - 1) & 1].p;
            if (int rc = launch(ctx, "k_tree_level", k_tree_level, lb, WG_BLOCK, st, src, l == 0 ? 1u : 0u, (const uint32_t *)b_ent.p,
                                (const uint32_t *)(d_off + (uint64_t)l * (S_cap + 1)), (const uint32_t *)(d_off + (uint64_t)(l + 1) * (S_cap + 1)),
                                maps + map_base, info[l], info[l + 1], rows, m, tw, (uint32_t *)b_lvl[l & 1].p,
                                (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
                return rc;
            map_base += info[l + 1];
        }
        unsigned hb;
        if (int rc = compose_blocks((uint64_t)rows * p * 2, &hb)) return rc;
        ProfScope ps(ctx, "k_scal_matmul_wnaf", st);
        if (int rc = launch_wg(ctx, k_scal_matmul_wnaf3, k_scal_matmul_wnaf, "k_scal_matmul_wnaf3", nullptr, hb, st,
                               (const uint32_t *)b_lvl[(T - 1) & 1].p, (const uint32_t *)b_ops.p, (const uint32_t *)b_cnt.p, rcap_h, (const uint32_t *)d_zero,
                               (uint32_t *)d_out + (uint64_t)r0 * p * 2 * REC_WORDS, rows, info[T] ? info[T] : 1u, p, 1u, 1u,
                               (const uint32_t *)ctx->d_one, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
            return rc;
    }
    *taken = true;
    return COFHE_HIP_OK;
}

// The chains route: segmented lockstep chains, one per output form and segment.
int matmul_chains_route(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_exp, const void *d_zero, void *d_out, uint32_t n, uint32_t m, uint32_t p,
                        uint32_t w, uint32_t exp_bits, hipStream_t st) {
    const uint64_t nbase = (uint64_t)n * m * 2, n_exps = (uint64_t)m * p;
    const uint32_t tw = 1u << (w - 2);
    // few outputs (the reference's own benchmark shape is 8 x 64 . 64 x 64): cut the inner dimension into
    // segments so that the chains fill the GPU, then fold the partial products with the accumulation tree
    uint32_t segs = 1;
    const uint64_t out_forms = (uint64_t)n * p * 2;
    if (out_forms < 32768 && m >= 8) {                        // 32768 chains = 4 workgroups on each of 256 CUs
        const uint64_t want = (32768 + out_forms - 1) / out_forms;
        segs = (uint32_t)(want < 16 ? want : 16);
        if (segs > m / 4) segs = m / 4;
        if (segs < 2) segs = 1;
    }
    if (ctx->opt_matmul_segments >= 1 && ctx->opt_matmul_segments <= m) segs = ctx->opt_matmul_segments;
    // workspace: plan_scal_matmul -- tables (tw > 1), digits, maxlen, schedules (rcap words per column), their lengths,
    // partial products and their tree (segs > 1)
    const uint32_t ncols = segs * p;
    const uint32_t rcap = matmul_rcap(exp_bits, m, segs);
    const WsPlan mp_ = plan_scal_matmul(n, m, p, exp_bits, w, segs);
    if (int rc = ensure_workspace(ctx, mp_.total, st)) return rc;
    uint8_t *ws = (uint8_t *)ctx->workspace;
    int8_t *digits = (int8_t *)(ws + mp_.off("digits"));
    uint32_t *maxlen = (uint32_t *)(ws + mp_.off("maxlen"));
    uint32_t *ops = (uint32_t *)(ws + mp_.off("ops"));
    uint32_t *counts = (uint32_t *)(ws + mp_.off("counts"));
    uint32_t *partial = (uint32_t *)(ws + mp_.off("partial"));
    HIPCHK(hipMemsetAsync(digits, 0, mp_.off("maxlen") + 256 - mp_.off("digits"), st));
    if (int rc = wnaf_digits(ctx, d_exp, n_exps, w, digits, maxlen, st)) return rc;
    if (int rc = launch(ctx, nullptr, k_matmul_schedule, ncols, 64, st, (const int8_t *)digits, (const uint32_t *)maxlen, m, p, segs, rcap, ops,
                        counts, ctx->d_status))
        return rc;
    const uint32_t *table;
    if (int rc = pow_table(ctx, d_cts, nbase, tw, ws + mp_.off("table"), st, &table)) return rc;
    unsigned mblocks;
    if (int rc = compose_blocks(out_forms * segs, &mblocks)) return rc;
    {
        ProfScope ps(ctx, "k_scal_matmul_wnaf", st);
        if (int rc = launch_wg(ctx, k_scal_matmul_wnaf3, k_scal_matmul_wnaf, "k_scal_matmul_wnaf3", nullptr, mblocks, st, table, (const uint32_t *)ops,
                               (const uint32_t *)counts, rcap, (const uint32_t *)d_zero, segs > 1 ? partial : (uint32_t *)d_out, n, m, p, tw, segs,
                               (const uint32_t *)ctx->d_one, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
            return rc;
    }
    if (segs > 1)
        return accumulate_impl(ctx, partial, d_zero, d_out, n, segs, p, ws + mp_.off("tree"), st);
    return COFHE_HIP_OK;
}
}  // namespace

int cofhe_hip_scal_matmul_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_exp, const void *d_zero,
                                  void *d_out, uint32_t n, uint32_t m, uint32_t p, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if ((uint64_t)n * p == 0) return COFHE_HIP_OK;
    unsigned blocks;
    if (int rc = compose_blocks((uint64_t)n * p * 2, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    WsUse use(ctx, st);
    // window width (wnaf_auto_width): a base's table is used by the p columns of its row
    const uint64_t nbase = (uint64_t)n * m * 2;
    uint32_t w = 2, exp_bits = 0;                              // exp_bits: longest exponent of the call
    if (m > 0) {
        // per base: 2^(w-2) compositions for the table, then ~bits/(w+1) per column -- needs the exponent length
        if (int rc = max_exp_bits(ctx, d_exp, (uint64_t)m * p, st, &exp_bits)) return rc;
        if (int rc = wnaf_auto_width(ctx, nbase, (double)p, exp_bits, &w)) return rc;
    }
    if (m >= (1u << 21)) return fail(COFHE_HIP_EINVAL, "inner dimension beyond 2^21");
    // The product-tree form (matmul_tree_route) when there is something to pair up and enough outputs for the Horner
    // chains to fill the GPU; small products keep the segmented lockstep chains (matmul_chains_route), which measured faster there
    // (profiles/r04_a/tree_time.txt: 8x64.64x64 11.7 vs 12.8 ms, 64^3 21.6 vs 20.9, 32x256.256x256 k-bit 683 vs 673,
    // 256^3 884 vs 787 ms -- chains vs tree).  "matmul_tree" = 0 / 1 pins the choice.
    const bool use_tree = ctx->opt_matmul_tree == 1 || (ctx->opt_matmul_tree == -1 && m >= 8 && (uint64_t)n * p * 2 >= 4096);
    if (use_tree && m > 0) {
        bool taken = false;
        if (int rc = matmul_tree_route(ctx, d_cts, d_exp, d_zero, d_out, n, m, p, w, exp_bits, st, &taken)) return rc;
        if (taken) return COFHE_HIP_OK;
    }
    return matmul_chains_route(ctx, d_cts, d_exp, d_zero, d_out, n, m, p, w, exp_bits, st);
}

namespace {
// the one launch site of k_transpose_records: out (cols x rows) = in (rows x cols)^T, elements of `words` words; 16-byte pieces
// when both pointers and the element size allow them (a caller's pointer is only known to be 4-byte aligned)
int transpose_launch(cofhe_hip_ctx *ctx, const void *d_in, void *d_out, uint32_t rows, uint32_t cols, uint32_t words, hipStream_t st) {
    const PieceGrid g = piece_grid((uint64_t)rows * cols, words, 256, {d_in, d_out});
    if (g.total == 0) return COFHE_HIP_OK;
    return launch(ctx, nullptr, k_transpose_records, g.blocks, 256, st, (const uint32_t *)d_in, (uint32_t *)d_out, rows, cols, words, g.flag());
}
// out (n x p) = zero o s (n x m) . cts (m x p) with s^T (m x n exponent records) as given -- by a transposition
// (cofhe_hip_matmul_plain_ct_records) or written transposed in the first place (cofhe_hip_conv2d_ct_filters_records):
// out^T (p x n) = cts^T (p x m) . s^T through cofhe_hip_scal_matmul_records, whose routes, width choice, options and
// synchronisations are the call's.  The two temporaries come from the block cache and go back behind the work queued on
// `stream`.  The caller holds the context lock, has set the device and has checked n p > 0, m < 2^21 and the launch limit.
int plain_ct_transposed(cofhe_hip_ctx *ctx, const void *d_st, const void *d_cts, const void *d_zero, void *d_out, uint32_t n, uint32_t m, uint32_t p,
                        void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const size_t cts_bytes = (size_t)m * p * CT_BYTES;
    DevBuf cts_t(stream), out_t(stream);         // cts^T (p x m), out^T (p x n)
    if (int rc = cts_t.get(ctx, cts_bytes ? cts_bytes : 4)) return rc;
    if (int rc = out_t.get(ctx, (size_t)n * p * CT_BYTES)) return rc;
    if (int rc = transpose_launch(ctx, d_cts, cts_t.p, m, p, 2 * REC_WORDS, st)) return rc;
    if (int rc = cofhe_hip_scal_matmul_records(ctx, cts_t.p, d_st, d_zero, out_t.p, p, m, n, stream)) return rc;
    return transpose_launch(ctx, out_t.p, d_out, p, n, 2 * REC_WORDS, st);
}
}  // namespace

// Needs no workspace plan of its own: the temporaries are three blocks of the block cache, and the product it calls carves
// the workspace by its own plans ("scal_matmul", "scal_matmul_tree") for the transposed shape (p, m, n).
int cofhe_hip_matmul_plain_ct_records(cofhe_hip_ctx *ctx, const void *d_s, const void *d_cts, const void *d_zero, void *d_out, uint32_t n,
                                      uint32_t m, uint32_t p, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if ((uint64_t)n * p == 0) return COFHE_HIP_OK;
    const size_t s_bytes = (size_t)n * m * EXP_BYTES;
    if (!clear_of({d_out, (size_t)n * p * CT_BYTES}, {{d_cts, (size_t)m * p * CT_BYTES}, {d_s, s_bytes}, {d_zero, CT_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "matmul_plain_ct: the output overlaps an input");
    if (m >= (1u << 21)) return fail(COFHE_HIP_EINVAL, "inner dimension beyond 2^21");
    unsigned blocks;
    if (int rc = compose_blocks((uint64_t)n * p * 2, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    DevBuf s_t(stream);                          // s^T (m x n)
    if (int rc = s_t.get(ctx, s_bytes ? s_bytes : 4)) return rc;
    if (int rc = transpose_launch(ctx, d_s, s_t.p, n, m, EXP_REC_WORDS, st)) return rc;
    return plain_ct_transposed(ctx, s_t.p, d_cts, d_zero, d_out, n, m, p, stream);
}

namespace {
ConvShape conv_shape_of(const cofhe_hip_conv2d_shape &a) {
    return ConvShape{a.B, a.H, a.W, a.C, a.kh, a.kw, a.Co, a.sh, a.sw, a.ph, a.pw, 0u, 0u};
}
ConvShape conv_geometry_of(const cofhe_hip_conv2d_geometry &a) {      // (no overloads: this file is extern "C")
    return ConvShape{a.B, a.H, a.W, a.C, a.kh, a.kw, a.Co, a.sh, a.sw, a.ph, a.pw, 0u, 0u, a.dh, a.dw, a.groups};
}
// the one launch site of k_gather_patches: the n x m patch matrix of the image (im2col), the principal form in the padding;
// 16-byte pieces when both pointers allow them (a caller's pointer is only known to be 4-byte aligned).  s has no groups: the
// patch matrix is dense over C
int gather_patches_launch(cofhe_hip_ctx *ctx, const ConvShape &s, const void *d_cts, void *d_patches, hipStream_t st) {
    const uint32_t n = conv_rows(s), m = conv_inner(s);
    const PieceGrid g = piece_grid((uint64_t)n * m * 2, REC_WORDS, 256, {d_cts, d_patches});
    if (g.total == 0) return COFHE_HIP_OK;
    return launch(ctx, "k_gather_patches", k_gather_patches, g.blocks, 256, st, s, (const uint32_t *)d_cts, (const uint32_t *)ctx->d_one,
                  (uint32_t *)d_patches, n, m, g.flag());
}
// the one launch site of k_expand_group_filters: the dense [kh, kw, C, Co] exponent tensor of the grouped filters d_w
// [kh, kw, C / groups, Co] into d_dense (a block of the block cache), the zero exponent outside the blocks
int expand_group_filters_launch(cofhe_hip_ctx *ctx, const ConvShape &s, const void *d_w, void *d_dense, hipStream_t st) {
    const PieceGrid g = piece_grid((uint64_t)s.kh * s.kw * s.C * s.Co, EXP_REC_WORDS, 256, {d_w});
    if (g.total == 0) return COFHE_HIP_OK;
    return launch(ctx, "k_expand_group_filters", k_expand_group_filters, g.blocks, 256, st, (const uint32_t *)d_w, (uint32_t *)d_dense, s.kh * s.kw,
                  s.C, s.Co, s.groups, g.flag());
}

// THE convolution, behind every entry point: the full geometry, validated here before the context or a pointer is looked at.
// Two routes.  Direct: the product-tree route of the matrix product with the table built once over the image and level 0
// reading its leaves through conv_leaf (plans "conv2d", "conv2d_grouped"), m = kh kw C / groups.  Gather: the patch matrix into
// a block of the block cache, then cofhe_hip_scal_matmul_records unchanged (its own plans) -- when the direct route declines or
// is pinned off.  The patch matrix is dense over C, so with groups the gather route first expands the filters to the dense
// [kh, kw, C, Co] tensor (k_expand_group_filters) and then costs what the block-diagonal filter always cost: `groups` times
// the digits, the segment scans and the patch matrix of the direct route.
int conv2d_run(cofhe_hip_ctx *ctx, const void *d_w, const void *d_cts, const void *d_zero, void *d_out, ConvShape s, void *stream) {
    if (const char *why = conv_shape_check(s)) return fail(COFHE_HIP_EINVAL, why);
    const uint32_t n = conv_rows(s), m = conv_inner(s), p = s.Co;
    if ((uint64_t)n * p == 0) return COFHE_HIP_OK;
    if (!clear_of({d_out, (size_t)n * p * CT_BYTES},
                  {{d_cts, (size_t)s.B * s.H * s.W * s.C * CT_BYTES}, {d_w, (size_t)m * p * EXP_BYTES}, {d_zero, CT_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "conv2d: the output overlaps an input");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const CombState &opt = comb_state(ctx);
    const bool grouped = s.groups > 1;
    // the gather route works on the dense inner dimension: kh kw C < 2^21 and the dense patch matrix within the formats' bound
    const uint64_t m_dense = (uint64_t)s.kh * s.kw * s.C;
    const bool gather_fits = !grouped || (m_dense < (1ull << 21) && (uint64_t)n * m_dense <= CONV_PATCH_LIMIT);
    // automatic: the direct route where the matrix product itself takes its tree (something to pair up, enough outputs for the
    // Horner chains to fill the GPU); small convolutions keep the chains, behind the gather.  With groups the direct route
    // wherever it does not decline: the gather pays `groups` times the patch matrix, the digits and the scans there
    // (DESIGN.md section 5 has the measurements)
    const bool direct = opt.opt_conv_route == 1 || !gather_fits || (opt.opt_conv_route == 0 && (grouped || (m >= 8 && (uint64_t)n * p * 2 >= 4096)));
    if (direct && m > 0) {
        WsUse use(ctx, st);
        // window width: the table of a pixel is used by the columns of its group in every window the pixel is in
        const uint64_t reuse = (uint64_t)((s.kh + s.sh - 1) / s.sh) * ((s.kw + s.sw - 1) / s.sw);
        uint32_t w = 2, exp_bits = 0;
        if (int rc = max_exp_bits(ctx, d_w, (uint64_t)m * p, st, &exp_bits)) return rc;
        if (int rc = wnaf_auto_width(ctx, (uint64_t)s.B * s.H * s.W * s.C * 2, (double)reuse * (p / s.groups), exp_bits, &w)) return rc;
        bool taken = false;
        if (int rc = matmul_tree_route(ctx, d_cts, d_w, d_zero, d_out, n, m, p, w, exp_bits, st, &taken, &s, opt.opt_conv_chunk_rows)) return rc;
        if (taken) return COFHE_HIP_OK;
    }
    if (!gather_fits)
        return fail(COFHE_HIP_EINVAL, "conv2d: the direct route declined and the dense patch matrix of the gather route does not fit");
    const ConvShape ds = conv_dense(s);
    DevBuf patches(stream), dense(stream);
    const size_t patch_bytes = (size_t)n * m_dense * CT_BYTES;
    if (int rc = patches.get(ctx, patch_bytes ? patch_bytes : 4)) return rc;
    if (int rc = gather_patches_launch(ctx, ds, d_cts, patches.p, st)) return rc;
    if (grouped) {
        const size_t dense_bytes = (size_t)m_dense * p * EXP_BYTES;
        if (int rc = dense.get(ctx, dense_bytes ? dense_bytes : 4)) return rc;
        if (int rc = expand_group_filters_launch(ctx, s, d_w, dense.p, st)) return rc;
    }
    return cofhe_hip_scal_matmul_records(ctx, patches.p, grouped ? dense.p : d_w, d_zero, d_out, n, (uint32_t)m_dense, p, stream);
}
// the one launch site of k_gather_patch_exponents: the m x n TRANSPOSED patch matrix of the plaintext image d_img (exponent
// records), the zero exponent in the padding; 16-byte pieces when both pointers allow them.  s has no groups
int gather_patch_exponents_launch(cofhe_hip_ctx *ctx, const ConvShape &s, const void *d_img, void *d_st, hipStream_t st) {
    const uint32_t n = conv_rows(s), m = conv_inner(s);
    const PieceGrid g = piece_grid((uint64_t)n * m, EXP_REC_WORDS, 256, {d_img, d_st});
    if (g.total == 0) return COFHE_HIP_OK;
    return launch(ctx, "k_gather_patch_exponents", k_gather_patch_exponents, g.blocks, 256, st, s, (const uint32_t *)d_img, (uint32_t *)d_st, n, m,
                  g.flag());
}
// what the two entry points with a PLAINTEXT image check before the context or a pointer is looked at: the geometry, and that
// it has no groups (with groups the patch matrix differs per column group); fills Ho, Wo
const char *conv_plain_image_check(ConvShape &s) {
    if (const char *why = conv_shape_check(s)) return why;
    return s.groups != 1 ? "conv2d: a plaintext image (ciphertext filters, the plaintext convolution) takes groups = 1" : nullptr;
}
// a pooling geometry: one filter per channel
ConvShape pool_shape_of(const cofhe_hip_conv2d_geometry &a) {
    ConvShape s = conv_geometry_of(a);
    s.Co = s.C;
    s.groups = s.C ? s.C : 1;
    return s;
}
// the body of the two out_shape entries
int conv_out_shape(ConvShape s, uint32_t *Ho, uint32_t *Wo) {
    if (const char *why = conv_shape_check(s)) return fail(COFHE_HIP_EINVAL, why);
    *Ho = s.Ho;
    *Wo = s.Wo;
    return COFHE_HIP_OK;
}
}  // namespace

int cofhe_hip_conv2d_out_shape(const cofhe_hip_conv2d_shape *shape, uint32_t *Ho, uint32_t *Wo) {
    if (!shape || !Ho || !Wo) return fail(COFHE_HIP_EINVAL, "null argument");
    return conv_out_shape(conv_shape_of(*shape), Ho, Wo);
}
int cofhe_hip_conv2d_geometry_out_shape(const cofhe_hip_conv2d_geometry *geometry, uint32_t *Ho, uint32_t *Wo) {
    if (!geometry || !Ho || !Wo) return fail(COFHE_HIP_EINVAL, "null argument");
    return conv_out_shape(conv_geometry_of(*geometry), Ho, Wo);
}

int cofhe_hip_conv2d_plain_ct_records(cofhe_hip_ctx *ctx, const void *d_w, const void *d_cts, const void *d_zero, void *d_out,
                                      const cofhe_hip_conv2d_shape *shape, void *stream) {
    if (!shape) return fail(COFHE_HIP_EINVAL, "null argument");
    return conv2d_run(ctx, d_w, d_cts, d_zero, d_out, conv_shape_of(*shape), stream);          // dh = dw = groups = 1
}
int cofhe_hip_conv2d_grouped_plain_ct_records(cofhe_hip_ctx *ctx, const void *d_w, const void *d_cts, const void *d_zero, void *d_out,
                                              const cofhe_hip_conv2d_geometry *geometry, void *stream) {
    if (!geometry) return fail(COFHE_HIP_EINVAL, "null argument");
    return conv2d_run(ctx, d_w, d_cts, d_zero, d_out, conv_geometry_of(*geometry), stream);
}

// The depthwise convolution with [kh, kw, 1, C] filters of ones.  The filters are kh kw C exponent records made here, in a block
// of the block cache: every word zero but the lowest byte of each record.  At exp_bits = 1 the window width stays 2, no table is
// built, and the tree is kh kw - 1 compositions per output record plus the one with zero.
int cofhe_hip_sum_pool2d_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_zero, void *d_out,
                                 const cofhe_hip_conv2d_geometry *geometry, void *stream) {
    if (!geometry) return fail(COFHE_HIP_EINVAL, "null argument");
    ConvShape s = pool_shape_of(*geometry);
    if (const char *why = conv_shape_check(s)) return fail(COFHE_HIP_EINVAL, why);
    const uint64_t nout = (uint64_t)conv_rows(s) * s.Co;
    if (nout == 0) return COFHE_HIP_OK;
    if (!clear_of({d_out, nout * CT_BYTES}, {{d_cts, (size_t)s.B * s.H * s.W * s.C * CT_BYTES}, {d_zero, CT_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "sum_pool2d: the output overlaps an input");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const size_t n_w = (size_t)conv_inner(s) * s.Co;
    DevBuf ones(stream);
    if (int rc = ones.get(ctx, n_w * EXP_BYTES)) return rc;
    HIPCHK(hipMemsetAsync(ones.p, 0, n_w * EXP_BYTES, st));
    HIPCHK(hipMemset2DAsync(ones.p, EXP_BYTES, 1, 1, n_w, st));         // one byte per record: magnitude 1, sign word 0
    return conv2d_run(ctx, ones.p, d_cts, d_zero, d_out, s, stream);
}

int cofhe_hip_matmul_plain_plain_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint32_t n, uint32_t m, uint32_t p,
                                         uint32_t kbits, void *stream) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if ((uint64_t)n * p == 0) return COFHE_HIP_OK;
    if (!clear_of({d_out, (size_t)n * p * EXP_BYTES}, {{d_a, (size_t)n * m * EXP_BYTES}, {d_b, (size_t)m * p * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "matmul_plain_plain: the output overlaps an input");
    const uint32_t gx = (p + PMM_TILE - 1) / PMM_TILE, gy = (n + PMM_TILE - 1) / PMM_TILE;
    if (gy > 65535u) return fail(COFHE_HIP_EINVAL, "work size out of range");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, nullptr, k_plain_matmul, dim3(gx, gy), PMM_THREADS, st, (const uint32_t *)d_a, (const uint32_t *)d_b, (uint32_t *)d_out, n, m,
                  p, kbits);
}

// the one launch site of k_plain_conv2d
int cofhe_hip_conv2d_plain_plain_records(cofhe_hip_ctx *ctx, const void *d_img, const void *d_w, void *d_out,
                                         const cofhe_hip_conv2d_geometry *geometry, uint32_t kbits, void *stream) {
    if (!geometry) return fail(COFHE_HIP_EINVAL, "null argument");
    ConvShape s = conv_geometry_of(*geometry);
    if (const char *why = conv_plain_image_check(s)) return fail(COFHE_HIP_EINVAL, why);
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    const uint32_t n = conv_rows(s), m = conv_inner(s), p = s.Co;
    if ((uint64_t)n * p == 0) return COFHE_HIP_OK;
    if (!clear_of({d_out, (size_t)n * p * EXP_BYTES}, {{d_img, (size_t)s.B * s.H * s.W * s.C * EXP_BYTES}, {d_w, (size_t)m * p * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "conv2d_plain_plain: the output overlaps an input");
    const uint32_t gx = (n + PMM_TILE - 1) / PMM_TILE, gy = (p + PMM_TILE - 1) / PMM_TILE;
    if (gy > 65535u) return fail(COFHE_HIP_EINVAL, "work size out of range");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_plain_conv2d", k_plain_conv2d, dim3(gx, gy), PMM_THREADS, st, s, (const uint32_t *)d_img, (const uint32_t *)d_w,
                  (uint32_t *)d_out, kbits);
}

// Needs no workspace plan of its own, like cofhe_hip_matmul_plain_ct_records: the transposed patch matrix of the image is
// written straight into the block that product transposes its left operand into, and the rest is that product's
int cofhe_hip_conv2d_ct_filters_records(cofhe_hip_ctx *ctx, const void *d_img_exps, const void *d_filters_cts, const void *d_zero, void *d_out,
                                        const cofhe_hip_conv2d_geometry *geometry, void *stream) {
    if (!geometry) return fail(COFHE_HIP_EINVAL, "null argument");
    ConvShape s = conv_geometry_of(*geometry);
    if (const char *why = conv_plain_image_check(s)) return fail(COFHE_HIP_EINVAL, why);      // m < 2^21 and the launch limit among it
    const uint32_t n = conv_rows(s), m = conv_inner(s), p = s.Co;
    if ((uint64_t)n * p == 0) return COFHE_HIP_OK;
    if (!clear_of({d_out, (size_t)n * p * CT_BYTES},
                  {{d_img_exps, (size_t)s.B * s.H * s.W * s.C * EXP_BYTES}, {d_filters_cts, (size_t)m * p * CT_BYTES}, {d_zero, CT_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "conv2d_ct_filters: the output overlaps an input");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const size_t st_bytes = (size_t)n * m * EXP_BYTES;
    DevBuf s_t(stream);                          // S^T (m x n): the patch matrix of the image, transposed
    if (int rc = s_t.get(ctx, st_bytes ? st_bytes : 4)) return rc;
    if (int rc = gather_patch_exponents_launch(ctx, s, d_img_exps, s_t.p, st)) return rc;
    return plain_ct_transposed(ctx, s_t.p, d_filters_cts, d_zero, d_out, n, m, p, stream);
}

// ---- polynomial evaluation from one opened value (pow_dot.hip) -------------------------------------------------------------
static_assert(COFHE_HIP_POLY_MAX_DEGREE == POLY_MAX_DEGREE, "the header's bound is the kernel's");
// touches no shared state of the context (no workspace, no table, no flag word): no lock
int cofhe_hip_pow_dot_records(cofhe_hip_ctx *ctx, const void *d_bases, const void *d_exps, void *d_out, uint64_t n_ct, uint32_t d, void *stream) {
    if (d == 0 || d > (uint32_t)POLY_MAX_DEGREE) return fail(COFHE_HIP_EINVAL, "pow_dot: 1 <= d <= 8 bases per record");
    if (n_ct == 0) return COFHE_HIP_OK;
    if (!d_bases || !d_exps || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (n_ct > (1ull << 36)) return fail(COFHE_HIP_EINVAL, "work size out of range");
    // k_pow_dot keeps the running product in the output record
    if (!clear_of({d_out, n_ct * CT_BYTES}, {{d_bases, d * n_ct * CT_BYTES}, {d_exps, d * n_ct * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "pow_dot: the output overlaps an input");
    unsigned blocks;
    if (int rc = compose_blocks(2 * n_ct, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_pow_dot", k_pow_dot, blocks, WG_BLOCK, st, (const uint32_t *)d_bases, (const uint32_t *)d_exps, (uint32_t *)d_out, n_ct, d,
                  (const uint32_t *)ctx->d_one, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
}

int cofhe_hip_poly_shift_records(cofhe_hip_ctx *ctx, const void *d_coef, const void *d_x, void *d_q, uint64_t n, uint32_t d, uint32_t kbits,
                                 void *stream) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (d > (uint32_t)POLY_MAX_DEGREE) return fail(COFHE_HIP_EINVAL, "poly_shift: degree beyond 8");
    if (n == 0) return COFHE_HIP_OK;
    if (!d_coef || !d_x || !d_q) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint64_t blocks = (n + PSH_THREADS - 1) / PSH_THREADS;
    if (blocks > 0x7FFFFFFFull) return fail(COFHE_HIP_EINVAL, "work size out of range");
    if (!clear_of({d_q, (size_t)(d + 1) * n * EXP_BYTES}, {{d_coef, (size_t)(d + 1) * EXP_BYTES}, {d_x, n * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "poly_shift: the output overlaps an input");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_poly_shift", k_poly_shift, (unsigned)blocks, PSH_THREADS, st, (const uint32_t *)d_coef, (const uint32_t *)d_x,
                  (uint32_t *)d_q, n, d, kbits);
}

// Needs no workspace plan of its own: the d + 1 exponent tensors q_0 .. q_d are one block of the block cache, and the plaintext
// addend that closes the call carves the workspace by the plan "comb" (kind 3).
int cofhe_hip_poly_close_records(cofhe_hip_ctx *ctx, const void *d_coef, const void *d_e, const void *d_powers, const uint32_t *f_record,
                                 void *d_out, uint64_t n_ct, uint32_t d, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (d == 0 || d > (uint32_t)POLY_MAX_DEGREE) return fail(COFHE_HIP_EINVAL, "poly_close: 1 <= d <= 8");
    if (kbits > 32u * PMM_MAX_LIMBS) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (int rc = comb_check(3, n_ct, 0, kbits, 0, 0)) return rc;
    if (n_ct == 0) return COFHE_HIP_OK;
    if (!d_coef || !d_e || !d_powers || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n_ct * CT_BYTES}, {{d_powers, d * n_ct * CT_BYTES}, {d_coef, (d + 1) * EXP_BYTES}, {d_e, n_ct * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "poly_close: the output overlaps an input");
    DevBuf q(stream);                             // q_0 | q_1 .. q_d, power-major
    if (int rc = q.get(ctx, (size_t)(d + 1) * n_ct * EXP_BYTES)) return rc;
    if (int rc = cofhe_hip_poly_shift_records(ctx, d_coef, d_e, q.p, n_ct, d, kbits, stream)) return rc;
    if (int rc = cofhe_hip_pow_dot_records(ctx, d_powers, (const uint8_t *)q.p + n_ct * EXP_BYTES, d_out, n_ct, d, stream)) return rc;
    return cofhe_hip_add_plain_records(ctx, d_out, q.p, nullptr, nullptr, nullptr, f_record, d_out, n_ct, kbits, 0, stream);
}

// ---- division by public divisors from one opened value (divide.hip) --------------------------------------------------------
static_assert(COFHE_HIP_DIV_MAX_KBITS == PDV_MAX_KBITS, "the header's bound is the kernel's");
// touches no shared state of the context but the status word, which the kernel sets atomically: no lock
int cofhe_hip_divfloor_plain_records(cofhe_hip_ctx *ctx, const void *d_v, const void *d_div, uint64_t n_div, void *d_q, uint64_t n,
                                     uint32_t kbits, void *stream) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (n_div == 0 || n % n_div != 0) return fail(COFHE_HIP_EINVAL, "divfloor: the element count is a multiple of the divisor count, which is not 0");
    if (n == 0) return COFHE_HIP_OK;
    if (!d_v || !d_div || !d_q) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint64_t blocks = (n + PDV_GROUPS - 1) / PDV_GROUPS;
    if (blocks > 0x7FFFFFFFull) return fail(COFHE_HIP_EINVAL, "work size out of range");
    if (!clear_of({d_q, n * EXP_BYTES}, {{d_v, n * EXP_BYTES}, {d_div, n_div * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "divfloor: the output overlaps an input");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_plain_divfloor", k_plain_divfloor, (unsigned)blocks, PDV_THREADS, st, (const uint32_t *)d_v, (const uint32_t *)d_div, n_div,
                  (uint32_t *)d_q, n, kbits, ctx->d_status);
}

// Needs no workspace plan of its own: the quotients of the opened values are one block of the block cache, and the plaintext
// addend that closes the call carves the workspace by the plan "comb" (kind 3).
int cofhe_hip_div_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_div, uint64_t n_div, const void *d_rq, const uint32_t *f_record,
                                void *d_out, uint64_t n_ct, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (n_div == 0 || n_ct % n_div != 0) return fail(COFHE_HIP_EINVAL, "div_close: the element count is a multiple of the divisor count, which is not 0");
    if (int rc = comb_check(3, n_ct, 0, kbits, 0, 0)) return rc;
    if (n_ct == 0) return COFHE_HIP_OK;
    if (!d_e || !d_div || !d_rq || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n_ct * CT_BYTES}, {{d_rq, n_ct * CT_BYTES}, {d_e, n_ct * EXP_BYTES}, {d_div, n_div * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "div_close: the output overlaps an input");
    DevBuf q(stream);                             // e_q = floor(s(e) / D)
    if (int rc = q.get(ctx, n_ct * EXP_BYTES)) return rc;
    if (int rc = cofhe_hip_divfloor_plain_records(ctx, d_e, d_div, n_div, q.p, n_ct, kbits, stream)) return rc;
    return cofhe_hip_add_plain_records(ctx, d_rq, q.p, nullptr, nullptr, nullptr, f_record, d_out, n_ct, kbits, 0, stream);
}

// ---- exact floor division by small public divisors from one opened value (divide_exact.hip) ---------------------------------
static_assert(COFHE_HIP_DIVX_MAX_ROWS == DIVX_MAX_ROWS, "the header's bound is the kernels'");
namespace {
// what every exact-division entry point refuses before it looks at a pointer: k, the tuple length, and element i reading
// divisor i mod n_div
int divx_check(uint32_t kbits, uint32_t rows, uint64_t n_div, uint64_t n) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (rows == 0 || rows > DIVX_MAX_ROWS) return fail(COFHE_HIP_EINVAL, "divx: a tuple has 1 <= rows <= 4096 entries");
    if (n_div == 0 || n % n_div != 0) return fail(COFHE_HIP_EINVAL, "divx: the element count is a multiple of the divisor count, which is not 0");
    if (n > (1ull << 36) / DIVX_MAX_ROWS) return fail(COFHE_HIP_EINVAL, "divx: too many items");
    return COFHE_HIP_OK;
}
}  // namespace
// touches no shared state of the context but the status word, which the kernel sets atomically: no lock
int cofhe_hip_divmod_plain_records(cofhe_hip_ctx *ctx, const void *d_v, const void *d_div, uint64_t n_div, void *d_q, void *d_rem, uint64_t n,
                                   uint32_t rows, uint32_t kbits, void *stream) {
    if (int rc = divx_check(kbits, rows, n_div, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_v || !d_div || !d_q || !d_rem) return fail(COFHE_HIP_EINVAL, "null argument");
    const Span v{d_v, n * EXP_BYTES}, div{d_div, n_div * EXP_BYTES}, q{d_q, n * EXP_BYTES}, rem{d_rem, n * 4};
    if (!clear_of(q, {v, div}) || !clear_of(rem, {v, div}) || !clear_of(rem, {q}))
        return fail(COFHE_HIP_EINVAL, "divmod: an output overlaps an input or the other output");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const unsigned blocks = (unsigned)((n + PDV_GROUPS - 1) / PDV_GROUPS);       // n <= 2^24: divx_check
    return launch(ctx, "k_plain_divmod", k_plain_divmod, blocks, PDV_THREADS, st, (const uint32_t *)d_v, (const uint32_t *)d_div, n_div,
                  (uint32_t *)d_q, (uint32_t *)d_rem, n, rows, kbits, ctx->d_status);
}

// the blocks of the divmod pass are one block of the block cache; the lock is held for it
int cofhe_hip_divx_rows_records(cofhe_hip_ctx *ctx, const void *d_r, const void *d_div, uint64_t n_div, void *d_out, uint64_t n, uint32_t rows,
                                uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = divx_check(kbits, rows, n_div, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_r || !d_div || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n * rows * EXP_BYTES}, {{d_r, n * EXP_BYTES}, {d_div, n_div * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "divx_rows: the output overlaps an input");
    DevBuf prep(stream);                          // q(r) | q(r) + 1 | (D - m(r), D) per element
    if (int rc = prep.get(ctx, n * DIVX_PREP_WORDS * 4)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    if (int rc = launch(ctx, "k_divx_prep", k_divx_prep, (unsigned)((n + PDV_GROUPS - 1) / PDV_GROUPS), PDV_THREADS, st, (const uint32_t *)d_r,
                        (const uint32_t *)d_div, n_div, (uint32_t *)prep.p, n, rows, kbits, ctx->d_status))
        return rc;
    const PieceGrid g = piece_grid(n * rows, EXP_REC_WORDS, DIVX_ROWS_THREADS, {d_out, prep.p});
    return launch(ctx, "k_divx_rows", k_divx_rows, g.blocks, DIVX_ROWS_THREADS, st, (const uint32_t *)prep.p, (uint32_t *)d_out, n, rows, g.flag());
}

// Needs no workspace plan of its own: the rows are one block of the block cache, and the fresh encryption that follows carves
// the workspace by the plan "comb" (kind 1) over n rows plaintexts.
int cofhe_hip_divx_tuples_records(cofhe_hip_ctx *ctx, const void *d_r, const void *d_div, uint64_t n_div, const void *d_rho,
                                  const uint32_t *h_record, const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n,
                                  uint32_t rows, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = divx_check(kbits, rows, n_div, n)) return rc;
    if (int rc = comb_check(1, n * rows, 0, kbits, 0, 0)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_r || !d_div || !d_rho || !h_record || !pk_record || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n * rows * CT_BYTES}, {{d_r, n * EXP_BYTES}, {d_div, n_div * EXP_BYTES}, {d_rho, n * rows * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "divx_tuples: the output overlaps an input");
    // T_j = q(r) + [m(r) + j >= D], the plaintexts of the tuples
    return encrypt_rows(ctx, n * rows, kbits, d_rho, h_record, pk_record, f_record, d_out, stream,
                        [&](void *d_rows) { return cofhe_hip_divx_rows_records(ctx, d_r, d_div, n_div, d_rows, n, rows, kbits, stream); });
}

// Needs no workspace plan of its own: the quotients and the remainders of the opened values are one block of the block cache,
// and the plaintext addend that closes the call carves the workspace by the plan "comb" (kind 3).
int cofhe_hip_divx_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_div, uint64_t n_div, const void *d_tuples, uint32_t rows,
                                 const uint32_t *f_record, void *d_out, uint64_t n, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = divx_check(kbits, rows, n_div, n)) return rc;
    if (int rc = comb_check(3, n, 0, kbits, 0, 0)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_e || !d_div || !d_tuples || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n * CT_BYTES}, {{d_tuples, n * rows * CT_BYTES}, {d_e, n * EXP_BYTES}, {d_div, n_div * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "divx_close: the output overlaps an input");
    DevBuf qm(stream);                            // q(e): n exponent records, then m(e): n words
    if (int rc = qm.get(ctx, n * EXP_BYTES + n * 4)) return rc;
    uint32_t *d_rem = (uint32_t *)((uint8_t *)qm.p + n * EXP_BYTES);
    if (int rc = cofhe_hip_divmod_plain_records(ctx, d_e, d_div, n_div, qm.p, d_rem, n, rows, kbits, stream)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const unsigned blocks = (unsigned)((n + DIVX_SELECT_WAVES - 1) / DIVX_SELECT_WAVES);        // n <= 2^24: divx_check
    if (int rc = launch(ctx, "k_divx_select", k_divx_select, blocks, DIVX_SELECT_THREADS, st, (const uint32_t *)d_rem, (const uint32_t *)d_tuples,
                        (uint32_t *)d_out, n, rows, aligned16({d_tuples, d_out}) ? 1u : 0u, ctx->d_status))
        return rc;
    return cofhe_hip_add_plain_records(ctx, d_out, qm.p, nullptr, nullptr, nullptr, f_record, d_out, n, kbits, 0, stream);
}

// host only: the tuples of opened values of shape S are a tensor of shape S + [rows]
int cofhe_hip_divx_shape(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t *rows) {
    if (!rows || (ndim_e && !shape_e) || (ndim_t && !shape_t)) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint32_t *tail;
    if (!tail_shape(ndim_e, shape_e, ndim_t, shape_t, 1, &tail) || tail[0] == 0 || tail[0] > DIVX_MAX_ROWS)
        return fail(COFHE_HIP_ESHAPE, "divx_close: the tuples are a ciphertext tensor of e's shape and a last dimension of 1 <= rows <= 4096");
    *rows = tail[0];
    return COFHE_HIP_OK;
}

// ---- table lookups from one opened value (lut.hip) -------------------------------------------------------------------------
static_assert(COFHE_HIP_LUT_MAX_BITS == LUT_MAX_BITS, "the header's bound is the kernels'");
namespace {
// what every lookup entry point refuses before it looks at a pointer: the table width, and element i reading table i mod n_tab
int lut_check(uint32_t bits, uint64_t n_tab, uint64_t n) {
    if (bits == 0 || bits > LUT_MAX_BITS) return fail(COFHE_HIP_EINVAL, "lut: a table has 2^bits entries, 1 <= bits <= 12");
    if (n_tab == 0 || n % n_tab != 0) return fail(COFHE_HIP_EINVAL, "lut: the element count is a multiple of the table count, which is not 0");
    if (n > (1ull << 36)) return fail(COFHE_HIP_EINVAL, "lut: too many items");
    return COFHE_HIP_OK;
}
}  // namespace
// touches no shared state of the context: no lock.  16-byte pieces when the table and the output allow them (a caller's
// pointer is only known to be 4-byte aligned)
int cofhe_hip_lut_rotate_records(cofhe_hip_ctx *ctx, const void *d_table, uint64_t n_tab, const void *d_r, void *d_out, uint64_t n, uint32_t bits,
                                 void *stream) {
    if (int rc = lut_check(bits, n_tab, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_table || !d_r || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, (n << bits) * EXP_BYTES}, {{d_table, (n_tab << bits) * EXP_BYTES}, {d_r, n * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "lut_rotate: the output overlaps an input");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const PieceGrid g = piece_grid(n << bits, EXP_REC_WORDS, 256, {d_table, d_out});
    return launch(ctx, "k_lut_rotate", k_lut_rotate, g.blocks, 256, st, (const uint32_t *)d_table, n_tab, (const uint32_t *)d_r, (uint32_t *)d_out, n,
                  bits, g.flag());
}

// Needs no workspace plan of its own: the rotated rows are one block of the block cache, and the fresh encryption that follows
// carves the workspace by the plan "comb" (kind 1) over n 2^bits plaintexts.
int cofhe_hip_lut_tuples_records(cofhe_hip_ctx *ctx, const void *d_table, uint64_t n_tab, const void *d_r, const void *d_rho, const uint32_t *h_record,
                                 const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n, uint32_t bits, uint32_t kbits,
                                 void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = lut_check(bits, n_tab, n)) return rc;
    if (bits > kbits) return fail(COFHE_HIP_EINVAL, "lut: bits <= k");
    if (int rc = comb_check(1, n << bits, 0, kbits, 0, 0)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_table || !d_r || !d_rho || !h_record || !pk_record || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, (n << bits) * CT_BYTES}, {{d_table, (n_tab << bits) * EXP_BYTES}, {d_r, n * EXP_BYTES}, {d_rho, (n << bits) * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "lut_tuples: the output overlaps an input");
    // T_j = g[(j + r) mod 2^bits], the plaintexts of the tuples
    return encrypt_rows(ctx, n << bits, kbits, d_rho, h_record, pk_record, f_record, d_out, stream,
                        [&](void *d_rows) { return cofhe_hip_lut_rotate_records(ctx, d_table, n_tab, d_r, d_rows, n, bits, stream); });
}

// touches no shared state of the context: no lock.  One wavefront per output ciphertext, 16-byte pieces when the tuples and the
// output allow them
int cofhe_hip_lut_select_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_tuples, void *d_out, uint64_t n, uint32_t bits, void *stream) {
    if (int rc = lut_check(bits, 1, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_e || !d_tuples || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n * CT_BYTES}, {{d_e, n * EXP_BYTES}, {d_tuples, (n << bits) * CT_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "lut_select: the output overlaps an input");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + LUT_SELECT_WAVES - 1) / LUT_SELECT_WAVES, 0x7FFFFFFFull);      // grid-stride beyond that
    return launch(ctx, "k_lut_select", k_lut_select, blocks, LUT_SELECT_THREADS, st, (const uint32_t *)d_e, (const uint32_t *)d_tuples,
                  (uint32_t *)d_out, n, bits, aligned16({d_tuples, d_out}) ? 1u : 0u);
}

// host only: the tuples of opened values of shape S are a tensor of shape S + [2^bits]
int cofhe_hip_lut_tuples_shape_bits(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t *bits) {
    if (!bits || (ndim_e && !shape_e) || (ndim_t && !shape_t)) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint32_t *tail;
    uint32_t b = 0;
    if (tail_shape(ndim_e, shape_e, ndim_t, shape_t, 1, &tail))
        while (b <= LUT_MAX_BITS && (1u << b) != tail[0]) b++;
    if (b == 0 || b > LUT_MAX_BITS)          // b stays 0 for a tensor of another shape
        return fail(COFHE_HIP_ESHAPE, "lut_select: the tuples are a ciphertext tensor of e's shape and a last dimension of 2^bits, 1 <= bits <= 12");
    *bits = b;
    return COFHE_HIP_OK;
}

// ---- rearranging resident tensors: affine views and index gathers (view.hip, view.hpp) --------------------------------------
namespace {
// a descriptor of a dense row-major source of shape[ndim] with nothing mapped yet, and its closing step: the box is the whole
// destination
int view_begin(const uint64_t *shape, uint32_t ndim, cofhe_hip_view *v) {
    if (!v || (ndim && !shape)) return fail(COFHE_HIP_EINVAL, "null argument");
    if (ndim > (uint32_t)VIEW_MAX_DIMS) return fail(COFHE_HIP_EINVAL, "view: more than 8 axes");
    memset(v, 0, sizeof *v);
    v->src_ndim = ndim;
    for (uint32_t a = 0; a < ndim; a++) v->src_extent[a] = shape[a];
    return COFHE_HIP_OK;
}
int view_end(cofhe_hip_view *v) {
    for (uint32_t d = 0; d < v->out_ndim; d++) {
        v->dst_extent[d] = v->out_extent[d];
        v->dst_start[d] = 0;
    }
    if (const char *why = view_check(*v, nullptr, nullptr, nullptr, nullptr)) return fail(COFHE_HIP_EINVAL, why);
    return COFHE_HIP_OK;
}
// the grid of the two kernels for n records of `pieces` pieces: as many workgroups as one pass needs, 64 per CU at the most (the
// kernels stride beyond that), or the pin of "view_grid_blocks"
unsigned view_blocks(const cofhe_hip_ctx *ctx, uint64_t n, uint32_t pieces) {
    if (const uint32_t pin = comb_state(ctx).opt_view_grid_blocks) return pin;
    const uint64_t per = pieces >= 64u ? VIEW_WAVES : VIEW_THREADS / VIEW_GROUP;
    return (unsigned)std::min<uint64_t>((n + per - 1) / per, 64u * NUM_CUS);
}
}  // namespace

int cofhe_hip_view_check(const cofhe_hip_view *view, uint64_t *n_src, uint64_t *n_box, uint64_t *n_dst, int *needs_fill) {
    if (!view) return fail(COFHE_HIP_EINVAL, "null argument");
    if (const char *why = view_check(*view, n_src, n_box, n_dst, needs_fill)) return fail(COFHE_HIP_EINVAL, why);
    return COFHE_HIP_OK;
}
int cofhe_hip_view_permute(const uint64_t *shape, uint32_t ndim, const uint32_t *perm, cofhe_hip_view *view) {
    if (int rc = view_begin(shape, ndim, view)) return rc;
    if (ndim && !perm) return fail(COFHE_HIP_EINVAL, "null argument");
    uint32_t seen = 0;
    view->out_ndim = ndim;
    for (uint32_t d = 0; d < ndim; d++) {
        if (perm[d] >= ndim || (seen >> perm[d] & 1u)) return fail(COFHE_HIP_EINVAL, "view_permute: not a permutation of the axes");
        seen |= 1u << perm[d];
        view->out_extent[d] = shape[perm[d]];
        view->map[perm[d]][d] = 1;
    }
    return view_end(view);
}
int cofhe_hip_view_slice(const uint64_t *shape, uint32_t ndim, const int64_t *start, const int64_t *stop, const int64_t *step,
                         cofhe_hip_view *view) {
    if (int rc = view_begin(shape, ndim, view)) return rc;
    if (ndim && (!start || !stop || !step)) return fail(COFHE_HIP_EINVAL, "null argument");
    view->out_ndim = ndim;
    for (uint32_t d = 0; d < ndim; d++) {
        if (shape[d] > (1ull << 62)) return fail(COFHE_HIP_EINVAL, "view_slice: extent out of range");
        const int64_t n = (int64_t)shape[d], a = start[d], b = stop[d], s = step[d];
        if (s == 0 || s > INT32_MAX || s < -INT32_MAX) return fail(COFHE_HIP_EINVAL, "view_slice: a step is 0 or beyond 31 bits");
        const bool ok = s > 0 ? (a >= 0 && a <= n && b >= 0 && b <= n) : (b >= -1 && b <= n - 1 && a >= -1 && a <= n - 1);
        if (!ok) return fail(COFHE_HIP_EINVAL, "view_slice: a bound lies outside its axis");
        const uint64_t span = s > 0 ? (b > a ? (uint64_t)(b - a) : 0) : (a > b ? (uint64_t)(a - b) : 0), mag = (uint64_t)(s > 0 ? s : -s);
        view->out_extent[d] = (span + mag - 1) / mag;
        view->start[d] = a;
        view->map[d][d] = (int32_t)s;
    }
    return view_end(view);
}
int cofhe_hip_view_pad(const uint64_t *shape, uint32_t ndim, const uint64_t *lo, const uint64_t *hi, cofhe_hip_view *view) {
    if (int rc = view_begin(shape, ndim, view)) return rc;
    if (ndim && (!lo || !hi)) return fail(COFHE_HIP_EINVAL, "null argument");
    view->out_ndim = ndim;
    for (uint32_t d = 0; d < ndim; d++) {
        if (shape[d] > (1ull << 48) || lo[d] > (1ull << 48) || hi[d] > (1ull << 48)) return fail(COFHE_HIP_EINVAL, "view_pad: extent out of range");
        view->out_extent[d] = lo[d] + shape[d] + hi[d];
        view->start[d] = -(int64_t)lo[d];
        view->map[d][d] = 1;
    }
    return view_end(view);
}
int cofhe_hip_view_broadcast(const uint64_t *shape, uint32_t ndim, const uint64_t *out_shape, uint32_t out_ndim, cofhe_hip_view *view) {
    if (int rc = view_begin(shape, ndim, view)) return rc;
    if (out_ndim && !out_shape) return fail(COFHE_HIP_EINVAL, "null argument");
    if (out_ndim > (uint32_t)VIEW_MAX_DIMS || out_ndim < ndim) return fail(COFHE_HIP_EINVAL, "view_broadcast: the output has fewer axes than the source, or more than 8");
    view->out_ndim = out_ndim;
    for (uint32_t d = 0; d < out_ndim; d++) view->out_extent[d] = out_shape[d];
    for (uint32_t a = 0; a < ndim; a++) {
        const uint32_t d = out_ndim - ndim + a;
        if (shape[a] == out_shape[d])
            view->map[a][d] = 1;
        else if (shape[a] != 1)
            return fail(COFHE_HIP_EINVAL, "view_broadcast: a source extent is neither 1 nor the output's");
    }
    return view_end(view);
}
int cofhe_hip_view_window_taps(const cofhe_hip_conv2d_geometry *geometry, cofhe_hip_view *view) {
    if (!geometry || !view) return fail(COFHE_HIP_EINVAL, "null argument");
    ConvShape s = pool_shape_of(*geometry);
    if (const char *why = conv_shape_check(s)) return fail(COFHE_HIP_EINVAL, why);
    if ((s.sh | s.sw | s.dh | s.dw) > (uint32_t)INT32_MAX) return fail(COFHE_HIP_EINVAL, "view_window_taps: a stride or a dilation beyond 31 bits");
    const uint64_t shape[4] = {s.B, s.H, s.W, s.C};
    if (int rc = view_begin(shape, 4, view)) return rc;
    const uint64_t out[6] = {s.kh, s.kw, s.B, s.Ho, s.Wo, s.C};
    view->out_ndim = 6;
    for (int d = 0; d < 6; d++) view->out_extent[d] = out[d];
    view->map[0][2] = 1;                         // b
    view->map[1][0] = (int32_t)s.dh;             // y = oy sh + dy dh - ph
    view->map[1][3] = (int32_t)s.sh;
    view->start[1] = -(int64_t)s.ph;
    view->map[2][1] = (int32_t)s.dw;             // x = ox sw + dx dw - pw
    view->map[2][4] = (int32_t)s.sw;
    view->start[2] = -(int64_t)s.pw;
    view->map[3][5] = 1;                         // c
    return view_end(view);
}
int cofhe_hip_view_into(cofhe_hip_view *view, const uint64_t *dst_shape, const uint64_t *dst_start) {
    if (!view) return fail(COFHE_HIP_EINVAL, "null argument");
    if (view->out_ndim > (uint32_t)VIEW_MAX_DIMS) return fail(COFHE_HIP_EINVAL, "view: more than 8 axes");
    if (view->out_ndim && (!dst_shape || !dst_start)) return fail(COFHE_HIP_EINVAL, "null argument");
    cofhe_hip_view v = *view;
    for (uint32_t d = 0; d < v.out_ndim; d++) {
        v.dst_extent[d] = dst_shape[d];
        v.dst_start[d] = dst_start[d];
    }
    if (const char *why = view_check(v, nullptr, nullptr, nullptr, nullptr)) return fail(COFHE_HIP_EINVAL, why);
    *view = v;
    return COFHE_HIP_OK;
}

// touches no shared state of the context but the option pin: no lock.  One launch; the descriptor travels as a kernel argument
int cofhe_hip_view_records(cofhe_hip_ctx *ctx, const cofhe_hip_view *view, const void *d_src, const void *d_fill, void *d_dst, uint32_t words,
                           void *stream) {
    if (!ctx || !view) return fail(COFHE_HIP_EINVAL, "null argument");
    uint64_t n_src = 0, n_box = 0, n_dst = 0;
    int needs_fill = 0;
    if (const char *why = view_check(*view, &n_src, &n_box, &n_dst, &needs_fill)) return fail(COFHE_HIP_EINVAL, why);
    if (words == 0) return fail(COFHE_HIP_EINVAL, "view_records: a record of 0 words");
    if (needs_fill && !d_fill) return fail(COFHE_HIP_EINVAL, "view_records: the view reads outside its source and there is no fill record");
    if (n_box == 0) return COFHE_HIP_OK;
    if (!d_dst || (n_src && !d_src)) return fail(COFHE_HIP_EINVAL, "null argument");
    const size_t rec_bytes = (size_t)words * 4;
    if (!clear_of({d_dst, n_dst * rec_bytes}, {{d_src, n_src * rec_bytes}, {d_fill, d_fill ? rec_bytes : 0}}))
        return fail(COFHE_HIP_EINVAL, "view_records: the destination overlaps the source or the fill record");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const bool vec16 = words % 4 == 0 && aligned16({d_src, d_fill, d_dst});
    const unsigned blocks = view_blocks(ctx, n_box, vec16 ? words / 4 : words);
    return launch(ctx, "k_view_records", k_view_records, blocks, VIEW_THREADS, st, *view, (const uint32_t *)d_src, (const uint32_t *)d_fill,
                  (uint32_t *)d_dst, words, vec16 ? 1u : 0u);
}

int cofhe_hip_gather_records(cofhe_hip_ctx *ctx, const void *d_src, uint64_t n_src, const void *d_index, const void *d_fill, void *d_dst,
                             uint64_t n_out, uint32_t words, void *stream) {
    if (!ctx) return fail(COFHE_HIP_EINVAL, "null argument");
    if (words == 0) return fail(COFHE_HIP_EINVAL, "gather_records: a record of 0 words");
    if (n_src > COFHE_HIP_GATHER_KEEP || n_out > VIEW_MAX_ELEMENTS) return fail(COFHE_HIP_EINVAL, "gather_records: too many records");
    if (n_out == 0) return COFHE_HIP_OK;
    if (!d_dst || !d_index || (n_src && !d_src)) return fail(COFHE_HIP_EINVAL, "null argument");
    const size_t rec_bytes = (size_t)words * 4, out_bytes = n_out * rec_bytes;
    if (!clear_of({d_dst, out_bytes}, {{d_src, n_src * rec_bytes}, {d_index, n_out * 4}, {d_fill, d_fill ? rec_bytes : 0}}))
        return fail(COFHE_HIP_EINVAL, "gather_records: the destination overlaps the source, the indices or the fill record");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const bool vec16 = words % 4 == 0 && aligned16({d_src, d_fill, d_dst});
    const unsigned blocks = view_blocks(ctx, n_out, vec16 ? words / 4 : words);
    return launch(ctx, "k_gather_records", k_gather_records, blocks, VIEW_THREADS, st, (const uint32_t *)d_src, n_src, (const uint32_t *)d_index,
                  (const uint32_t *)d_fill, (uint32_t *)d_dst, n_out, words, vec16 ? 1u : 0u, ctx->d_status);
}

// ---- piecewise-polynomial activations from one opened value (spline.hip) ---------------------------------------------------
static_assert(COFHE_HIP_SPLINE_MAX_TUPLE == SPLINE_MAX_TUPLE, "the header's bound is the kernels'");
namespace {
// what every spline entry point refuses before it looks at a pointer: the window, the degree, the tuple size, and element i
// reading table i mod n_tab
int spline_check(uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits, uint64_t n_tab, uint64_t n) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (!spline_shape_ok(bits, shift, d, kbits))
        return fail(COFHE_HIP_EINVAL, "spline: 2^bits pieces of degree d, bits >= 1, 1 <= d <= 8, 2^bits (d + 1) <= 4096, shift + bits <= k");
    if (n_tab == 0 || n % n_tab != 0) return fail(COFHE_HIP_EINVAL, "spline: the element count is a multiple of the table count, which is not 0");
    if (n > (1ull << 36) / SPLINE_MAX_TUPLE) return fail(COFHE_HIP_EINVAL, "spline: too many items");
    return COFHE_HIP_OK;
}
}  // namespace
// touches no shared state of the context: no lock
int cofhe_hip_spline_rows_records(cofhe_hip_ctx *ctx, const void *d_pieces, uint64_t n_tab, const void *d_r, void *d_out, uint64_t n, uint32_t bits,
                                  uint32_t shift, uint32_t d, uint32_t kbits, void *stream) {
    if (int rc = spline_check(bits, shift, d, kbits, n_tab, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_pieces || !d_r || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    const size_t row_bytes = (size_t)(d + 1) * EXP_BYTES;
    if (!clear_of({d_out, (n << bits) * row_bytes}, {{d_pieces, (n_tab << bits) * row_bytes}, {d_r, n * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "spline_rows: the output overlaps an input");
    const uint64_t blocks = ((n << bits) + SPL_THREADS - 1) / SPL_THREADS;
    if (blocks > 0x7FFFFFFFull) return fail(COFHE_HIP_EINVAL, "work size out of range");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_spline_rows", k_spline_rows, (unsigned)blocks, SPL_THREADS, st, (const uint32_t *)d_pieces, n_tab, (const uint32_t *)d_r,
                  (uint32_t *)d_out, n, bits, shift, d, kbits);
}

// Needs no workspace plan of its own: the rows are one block of the block cache, and the fresh encryption that follows carves
// the workspace by the plan "comb" (kind 1) over n 2^bits (d + 1) plaintexts.
int cofhe_hip_spline_tuples_records(cofhe_hip_ctx *ctx, const void *d_pieces, uint64_t n_tab, const void *d_r, const void *d_rho,
                                    const uint32_t *h_record, const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n,
                                    uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = spline_check(bits, shift, d, kbits, n_tab, n)) return rc;
    const uint64_t per = (uint64_t)(d + 1) << bits;
    if (int rc = comb_check(1, n * per, 0, kbits, 0, 0)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_pieces || !d_r || !d_rho || !h_record || !pk_record || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n * per * CT_BYTES}, {{d_pieces, n_tab * per * EXP_BYTES}, {d_r, n * EXP_BYTES}, {d_rho, n * per * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "spline_tuples: the output overlaps an input");
    // q_{j,c}: the plaintexts of the tuples
    return encrypt_rows(ctx, n * per, kbits, d_rho, h_record, pk_record, f_record, d_out, stream, [&](void *d_rows) {
        return cofhe_hip_spline_rows_records(ctx, d_pieces, n_tab, d_r, d_rows, n, bits, shift, d, kbits, stream);
    });
}

// touches no shared state of the context: no lock
int cofhe_hip_spline_powers_records(cofhe_hip_ctx *ctx, const void *d_e, void *d_out, uint64_t n, uint32_t d, uint32_t kbits, void *stream) {
    if (int rc = spline_check(1, 0, d, kbits, 1, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_e || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, (size_t)d * n * EXP_BYTES}, {{d_e, n * EXP_BYTES}})) return fail(COFHE_HIP_EINVAL, "spline_powers: the output overlaps the input");
    const uint64_t blocks = (n + SPL_THREADS - 1) / SPL_THREADS;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_spline_powers", k_spline_powers, (unsigned)blocks, SPL_THREADS, st, (const uint32_t *)d_e, (uint32_t *)d_out, n, d, kbits);
}

// the powers of the opened values are one block of the block cache; the status word is set by the kernel through Ctx
int cofhe_hip_spline_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_tuples, void *d_out, uint64_t n, uint32_t bits,
                                   uint32_t shift, uint32_t d, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = spline_check(bits, shift, d, kbits, 1, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_e || !d_tuples || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, n * CT_BYTES}, {{d_e, n * EXP_BYTES}, {d_tuples, (((uint64_t)(d + 1) * n) << bits) * CT_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "spline_close: the output overlaps an input");
    unsigned blocks;
    if (int rc = compose_blocks(2 * n, &blocks)) return rc;
    DevBuf powers(stream);                        // e, e^2, .., e^d mod 2^k, power-major
    if (int rc = powers.get(ctx, (size_t)d * n * EXP_BYTES)) return rc;
    if (int rc = cofhe_hip_spline_powers_records(ctx, d_e, powers.p, n, d, kbits, stream)) return rc;      // makes the device current
    return launch(ctx, "k_spline_close", k_spline_close, blocks, WG_BLOCK, (hipStream_t)stream, (const uint32_t *)d_e, (const uint32_t *)powers.p,
                  (const uint32_t *)d_tuples, (uint32_t *)d_out, n, bits, shift, d, kbits, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits,
                  ctx->d_status);
}

// host only: the tuples of opened values of shape S are a tensor of shape S + [2^bits, d + 1]
int cofhe_hip_spline_tuples_shape(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t *bits, uint32_t *d) {
    if (!bits || !d || (ndim_e && !shape_e) || (ndim_t && !shape_t)) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint32_t *tail;
    uint32_t b = 0, dd = 0;
    if (tail_shape(ndim_e, shape_e, ndim_t, shape_t, 2, &tail)) {      // b stays 0 for a tensor of another shape
        while (b <= 12u && (1u << b) != tail[0]) b++;
        dd = tail[1] - 1u;                                       // 0 entries: wraps to a degree that is refused
    }
    if (b == 0 || b > 12u || dd == 0 || dd > (uint32_t)POLY_MAX_DEGREE || ((uint64_t)(dd + 1) << b) > SPLINE_MAX_TUPLE)
        return fail(COFHE_HIP_ESHAPE, "spline_close: the tuples are a ciphertext tensor of e's shape and two last dimensions [2^bits, d + 1], "
                                      "bits >= 1, 1 <= d <= 8, 2^bits (d + 1) <= 4096");
    *bits = b;
    *d = dd;
    return COFHE_HIP_OK;
}

// ---- the sign on a window of up to 64 bits from digit comparisons (compare.hip) ---------------------------------------------
static_assert(COFHE_HIP_CMP_MAX_BITS == CMP_MAX_BITS && COFHE_HIP_CMP_MAX_DIGIT_BITS == CMP_MAX_DIGIT_BITS, "the header's bounds are the kernels'");
static_assert(CMP_MAX_DIGITS + 1 == LUT_MAX_BITS, "the lookup that closes a comparison has n + 1 bits");
namespace {
// what every comparison entry point refuses before it looks at a pointer: the window, the digit width and the digit count
int cmp_check(uint32_t bits, uint32_t digit_bits, uint32_t kbits, uint64_t n) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    if (!cmp_shape_ok(bits, digit_bits, kbits, LUT_MAX_BITS))
        return fail(COFHE_HIP_EINVAL, "cmp: a window of 2 <= bits <= min(k, 64) bits in n = ceil(bits / d) digits of 1 <= d <= 8 bits, "
                                      "n + 1 <= min(12, k)");
    if (n > (1ull << 36) / (CMP_MAX_DIGITS << CMP_MAX_DIGIT_BITS)) return fail(COFHE_HIP_EINVAL, "cmp: too many items");
    return COFHE_HIP_OK;
}
}  // namespace
// touches no shared state of the context: no lock.  16-byte pieces when the output allows them (a caller's pointer is only known
// to be 4-byte aligned)
int cofhe_hip_cmp_rows_records(cofhe_hip_ctx *ctx, const void *d_r, void *d_out, uint64_t n, uint32_t bits, uint32_t digit_bits, uint32_t kbits,
                               void *stream) {
    if (int rc = cmp_check(bits, digit_bits, kbits, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_r || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint64_t recs = (n * cmp_digits(bits, digit_bits)) << digit_bits;
    if (!clear_of({d_out, recs * EXP_BYTES}, {{d_r, n * EXP_BYTES}})) return fail(COFHE_HIP_EINVAL, "cmp_rows: the output overlaps the input");
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    const PieceGrid g = piece_grid(recs, EXP_REC_WORDS, CMP_ROWS_THREADS, {d_out});
    return launch(ctx, "k_cmp_rows", k_cmp_rows, g.blocks, CMP_ROWS_THREADS, st, (const uint32_t *)d_r, (uint32_t *)d_out, n, bits, digit_bits, g.flag());
}

// Needs no workspace plan of its own: the rows are one block of the block cache, and the fresh encryption that follows carves
// the workspace by the plan "comb" (kind 1) over n nd 2^d plaintexts.
int cofhe_hip_cmp_tuples_records(cofhe_hip_ctx *ctx, const void *d_r, const void *d_rho, const uint32_t *h_record, const uint32_t *pk_record,
                                 const uint32_t *f_record, void *d_out, uint64_t n, uint32_t bits, uint32_t digit_bits, uint32_t kbits,
                                 void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = cmp_check(bits, digit_bits, kbits, n)) return rc;
    const uint64_t recs = (n * cmp_digits(bits, digit_bits)) << digit_bits;
    if (int rc = comb_check(1, recs, 0, kbits, 0, 0)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_r || !d_rho || !h_record || !pk_record || !f_record || !d_out) return fail(COFHE_HIP_EINVAL, "null argument");
    if (!clear_of({d_out, recs * CT_BYTES}, {{d_r, n * EXP_BYTES}, {d_rho, recs * EXP_BYTES}}))
        return fail(COFHE_HIP_EINVAL, "cmp_tuples: the output overlaps an input");
    // T[j][c] = 2^j sgn(r_j - c), the plaintexts of the tuples
    return encrypt_rows(ctx, recs, kbits, d_rho, h_record, pk_record, f_record, d_out, stream,
                        [&](void *d_rows) { return cofhe_hip_cmp_rows_records(ctx, d_r, d_rows, n, bits, digit_bits, kbits, stream); });
}

// no workspace and no block; the lock is held because the kernel sets the context's status word through Ctx, as k_spline_close
int cofhe_hip_cmp_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_tuples, void *d_out, void *d_wrap, uint64_t n, uint32_t bits,
                                uint32_t digit_bits, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (int rc = cmp_check(bits, digit_bits, kbits, n)) return rc;
    if (n == 0) return COFHE_HIP_OK;
    if (!d_e || !d_tuples || !d_out || !d_wrap) return fail(COFHE_HIP_EINVAL, "null argument");
    const uint64_t recs = (n * cmp_digits(bits, digit_bits)) << digit_bits;
    const Span e{d_e, n * EXP_BYTES}, tuples{d_tuples, recs * CT_BYTES}, out{d_out, 2 * n * CT_BYTES}, wrap{d_wrap, n * EXP_BYTES};
    if (!clear_of(out, {e, tuples}) || !clear_of(wrap, {e, tuples}) || !clear_of(wrap, {out}))
        return fail(COFHE_HIP_EINVAL, "cmp_close: an output overlaps an input or the other output");
    unsigned blocks;
    if (int rc = compose_blocks(2 * n, &blocks)) return rc;
    hipStream_t st;
    if (int rc = on_device(ctx, stream, &st)) return rc;
    return launch(ctx, "k_cmp_close", k_cmp_close, blocks, WG_BLOCK, st, (const uint32_t *)d_e, (const uint32_t *)d_tuples, (uint32_t *)d_out,
                  (uint32_t *)d_wrap, n, bits, digit_bits, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
}

// host only: nd and nd 2^d, and the tuples of opened values of shape S as a tensor of shape S + [nd, 2^d]
int cofhe_hip_cmp_shape(uint32_t bits, uint32_t digit_bits, uint32_t kbits, uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t,
                        const uint32_t *shape_t, uint32_t *digits, uint32_t *entries) {
    if (int rc = cmp_check(bits, digit_bits, kbits, 0)) return rc;
    const uint32_t nd = cmp_digits(bits, digit_bits);
    if (shape_t) {
        if (ndim_e && !shape_e) return fail(COFHE_HIP_EINVAL, "null argument");
        const uint32_t *tail;
        if (!tail_shape(ndim_e, shape_e, ndim_t, shape_t, 2, &tail) || tail[0] != nd || tail[1] != (1u << digit_bits))
            return fail(COFHE_HIP_ESHAPE, "cmp_close: the tuples are a ciphertext tensor of e's shape and two last dimensions "
                                          "[ceil(bits / d), 2^d]");
    }
    if (digits) *digits = nd;
    if (entries) *entries = nd << digit_bits;
    return COFHE_HIP_OK;
}

namespace {
// the table f^(-2^j), j < k, of the decryption kernels (built on first use, cached in the context)
int ensure_ftab(cofhe_hip_ctx *ctx, const uint32_t *f_record, uint32_t kbits, void *stream) {
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->ftab_k != kbits || memcmp(ctx->ftab_f, f_record, REC_WORDS * 4) != 0) {
        // ftab[2j], ftab[2j+1] = f^(-2^j): k "ciphertexts" (f, f) raised to -2^j by k_pow
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        if (ctx->d_ftab) HIPCHK(hipFree(ctx->d_ftab));
        ctx->d_ftab = nullptr;
        ctx->ftab_k = 0;
        std::vector<uint32_t> base((size_t)kbits * 2 * REC_WORDS), ex((size_t)kbits * EXP_REC_WORDS, 0);
        for (uint32_t j = 0; j < kbits; j++) {
            memcpy(&base[(size_t)(2 * j) * REC_WORDS], f_record, REC_WORDS * 4);
            memcpy(&base[(size_t)(2 * j + 1) * REC_WORDS], f_record, REC_WORDS * 4);
            ex[(size_t)j * EXP_REC_WORDS + (j >> 5)] = 1u << (j & 31);
            ex[(size_t)j * EXP_REC_WORDS + EXP_MAG_WORDS] = 1u;          // negative
        }
        struct Tmp { void *p = nullptr; ~Tmp() { if (p) (void)hipFree(p); } } db, de;
        HIPCHK(dev_alloc(ctx, &db.p, base.size() * 4));
        HIPCHK(dev_alloc(ctx, &de.p, ex.size() * 4));
        HIPCHK(dev_alloc(ctx, (void **)&ctx->d_ftab, base.size() * 4));
        HIPCHK(hipMemcpy(db.p, base.data(), base.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(de.p, ex.data(), ex.size() * 4, hipMemcpyHostToDevice));
        if (int rc = cofhe_hip_pow_records(ctx, db.p, de.p, ctx->d_ftab, kbits, nullptr)) return rc;
        HIPCHK(hipDeviceSynchronize());
        memcpy(ctx->ftab_f, f_record, REC_WORDS * 4);
        ctx->ftab_k = kbits;
    }
    return COFHE_HIP_OK;
}
// m = dlog(c2 o prod parts^-+1) for every ciphertext: the one launch of decryption and of the threshold combiner
int decrypt_launch(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_parts, uint32_t n_parts, uint64_t negmask, void *d_out, uint64_t n_ct,
                   uint32_t kbits, void *stream) {
    unsigned blocks;
    if (int rc = compose_blocks(n_ct, &blocks)) return rc;
    return launch_wg(ctx, k_decrypt3, k_decrypt, "k_decrypt3", "k_decrypt", blocks, (hipStream_t)stream, (const uint32_t *)d_cts,
                     (const uint32_t *)d_parts, n_parts, negmask, (const uint32_t *)ctx->d_ftab, (uint32_t *)d_out, n_ct, (int)kbits,
                     (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status);
}
}  // namespace

int cofhe_hip_decrypt_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_sk, const uint32_t *f_record,
                              void *d_out, uint64_t n_ct, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_ct == 0) return COFHE_HIP_OK;
    if (int rc = ensure_ftab(ctx, f_record, kbits, stream)) return rc;
    WsUse use(ctx, (hipStream_t)stream);
    // d = c1^sk for every ciphertext (windowed ladder), then m = dlog(c2 o d^-1): the combiner with one part, which
    // k_decrypt reads from the front of the workspace (plan "decrypt": front = one record per ciphertext)
    void *d_parts = nullptr;
    if (int rc = pow_shared_c1(ctx, d_cts, d_sk, nullptr, n_ct, (size_t)n_ct * REC_WORDS * 4, &d_parts, (hipStream_t)stream))
        return rc;
    return decrypt_launch(ctx, d_cts, d_parts, 1u, 0, d_out, n_ct, kbits, stream);
}

int cofhe_hip_encrypt_records(cofhe_hip_ctx *ctx, const void *d_plain, const void *d_c1_pkr, const uint32_t *f_record,
                              void *d_out, uint64_t n_ct, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_ct == 0) return COFHE_HIP_OK;
    if (int rc = ensure_ftab(ctx, f_record, kbits, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    WsUse use(ctx, st);
    // c2_i = pk^r o f^(m_i) is a product of table entries (one per non-zero signed digit of m_i, ~k/3 of them) and has
    // no squarings, so it is multiplied out as a pairwise TREE over all elements at once: log2 levels of independent
    // compositions (k_compose_pairs over the entry-major layout) instead of a lockstep chain of ~k/3 rounds.  Same
    // number of compositions; at 128x128 the chain kernel took 22 ms, one ciphertext 20 ms (latency of 45 rounds).
    const uint32_t cap = kbits / 2 + 3;                          // pk^r + at most ceil((k + 1) / 2) digits
    const uint64_t CHUNK = 65536;                                // elements per pass: bounds the workspace (cap x CHUNK records x 2)
    for (uint64_t e0 = 0; e0 < n_ct; e0 += CHUNK) {
        const uint64_t ne = n_ct - e0 < CHUNK ? n_ct - e0 : CHUNK;
        const WsPlan ep = plan_encrypt_chunk(ne, kbits);
        if (int rc = ensure_workspace(ctx, ep.total, st)) return rc;
        uint8_t *ws = (uint8_t *)ctx->workspace;
        uint64_t *d_tabs = (uint64_t *)(ws + ep.off("header"));   // [0] table of f, [1] (h^r, pk^r); [2] = the slot counter
        uint32_t *d_max = (uint32_t *)(ws + ep.off("header") + 16);
        uint32_t *d_idx = (uint32_t *)(ws + ep.off("idx"));
        uint32_t *buf[2] = {(uint32_t *)(ws + ep.off("level_a")), (uint32_t *)(ws + ep.off("level_b"))};
        const uint64_t tabs[3] = {(uint64_t)(uintptr_t)ctx->d_ftab, (uint64_t)(uintptr_t)d_c1_pkr, 0};
        HIPCHK(hipMemcpyAsync(d_tabs, tabs, sizeof(tabs), hipMemcpyHostToDevice, st));
        if (int rc = launch(ctx, nullptr, k_encrypt_select, (unsigned)((ne + 255) / 256), 256, st, (const uint32_t *)d_plain + e0 * EXP_REC_WORDS, ne,
                            (int)kbits, cap, d_idx, d_max))
            return rc;
        uint32_t mmax = 0;
        HIPCHK(hipMemcpyAsync(&mmax, d_max, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                        // also: `tabs` has been read
        if (mmax == 0 || mmax > cap) return fail(COFHE_HIP_EHIP, "encryption: slot count out of range");
        const uint64_t total = (uint64_t)mmax * ne;
        unsigned gblocks;
        if (int rc = compose_blocks(total, &gblocks)) return rc;
        if (int rc = launch(ctx, nullptr, k_gather_signed, gblocks, WG_BLOCK, st, (const uint64_t *)d_tabs, (const uint32_t *)d_idx, total,
                            (const uint32_t *)ctx->d_one, buf[0]))
            return rc;
        const uint32_t *c2;
        if (int rc = product_tree(ctx, buf[0], buf[1], buf[0], nullptr, 1u, mmax, (uint32_t)ne, nullptr, st, &c2)) return rc;
        const unsigned zblocks = (unsigned)std::min<uint64_t>((ne * 2 * REC_WORDS + 255) / 256, 4096);
        if (int rc = launch(ctx, nullptr, k_zip_ciphertexts, zblocks, 256, st, (const uint32_t *)d_c1_pkr, c2, ne, (uint32_t *)d_out + e0 * 2 * REC_WORDS))
            return rc;
    }
    return COFHE_HIP_OK;
}

int cofhe_hip_combine_part_decryptions_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_parts,
                                               uint32_t n_parts, const int32_t *lambda, const uint32_t *f_record,
                                               void *d_out, uint64_t n_ct, uint32_t kbits, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_parts == 0 || n_parts > 64) return fail(COFHE_HIP_EINVAL, "between 1 and 64 partial decryptions per ciphertext");
    uint64_t negmask = 0;
    for (uint32_t i = 0; i < n_parts; i++) {
        if (lambda[i] != 1 && lambda[i] != -1) return fail(COFHE_HIP_EINVAL, "reconstruction coefficients must be +1 or -1");
        if (lambda[i] < 0) negmask |= 1ull << i;
    }
    if (n_ct == 0) return COFHE_HIP_OK;
    if (int rc = ensure_ftab(ctx, f_record, kbits, stream)) return rc;
    return decrypt_launch(ctx, d_cts, d_parts, n_parts, negmask, d_out, n_ct, kbits, stream);
}

int cofhe_hip_time_compose(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n, int iters,
                           void *stream, float *ms_per_launch) {
    if (iters <= 0 || n == 0) return fail(COFHE_HIP_EINVAL, "iters and n must be positive");
    unsigned blocks;
    if (int rc = compose_blocks(n, &blocks)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, (hipStream_t)stream));
    for (int i = 0; i < iters; i++)      // what cofhe_hip_compose_records launches, without its span
        if (int rc = launch_wg(ctx, k_compose_wg3, k_compose_wg, nullptr, nullptr, blocks, (hipStream_t)stream, (const uint32_t *)d_a,
                               (const uint32_t *)d_b, (uint32_t *)d_out, n, (const uint32_t *)ctx->d_absdelta, ctx->half_dbits, ctx->d_status))
            return rc;
    HIPCHK(hipEventRecord(e1, (hipStream_t)stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    *ms_per_launch = ms / iters;
    return COFHE_HIP_OK;
}

int cofhe_hip_workspace_plan(const char *op, const uint64_t *args, uint32_t n_args, cofhe_hip_ws_region *regions, uint32_t cap,
                             uint32_t *n_regions, uint64_t *total_bytes) {
    if (!op || !args || !n_regions || !total_bytes) return fail(COFHE_HIP_EINVAL, "null argument");
    const std::string o(op);
    auto need = [&](uint32_t k) { return n_args == k; };
    WsPlan p;
    if (o == "pow_shared" && need(2)) {
        p = plan_pow_shared(args[0], (size_t)args[1]);
    } else if ((o == "decrypt" || o == "part_decrypt") && need(2)) {
        // pow_shared_c1: one ladder when the tensor shares its c1 (found out per call for n_ct >= 64), else one per ciphertext;
        // decryption keeps c1^sk of every ciphertext in front of the tables (k_decrypt reads it as its one "part")
        const uint64_t n_ct = args[0], ladders = (args[1] && n_ct >= 64) ? 1 : n_ct;
        p = plan_pow_shared(ladders, o == "decrypt" ? (size_t)n_ct * REC_WORDS * 4 : 0);
    } else if (o == "scal_matmul" && need(6)) {
        if (args[4] < 2 || args[4] > 8 || args[5] < 1) return fail(COFHE_HIP_EINVAL, "scal_matmul plan: w in 2..8, segs >= 1");
        p = plan_scal_matmul((uint32_t)args[0], (uint32_t)args[1], (uint32_t)args[2], (uint32_t)args[3], (uint32_t)args[4], (uint32_t)args[5]);
    } else if (o == "scal_matmul_tree" && need(5)) {
        if (args[4] < 2 || args[4] > 8) return fail(COFHE_HIP_EINVAL, "scal_matmul_tree plan: w in 2..8");
        p = plan_scal_matmul_tree((uint32_t)args[0], (uint32_t)args[1], (uint32_t)args[2], (uint32_t)args[3], (uint32_t)args[4]);
    } else if (o == "conv2d" && need(13)) {
        // B, H, W, C, kh, kw, Co, sh, sw, ph, pw, exp_bits, w: the direct route of cofhe_hip_conv2d_plain_ct_records
        for (int i = 0; i < 13; i++)
            if (args[i] > 0xFFFFFFFFull) return fail(COFHE_HIP_EINVAL, "conv2d plan: argument out of range");
        if (args[12] < 2 || args[12] > 8) return fail(COFHE_HIP_EINVAL, "conv2d plan: w in 2..8");
        ConvShape cs{(uint32_t)args[0], (uint32_t)args[1], (uint32_t)args[2], (uint32_t)args[3], (uint32_t)args[4], (uint32_t)args[5], (uint32_t)args[6],
                     (uint32_t)args[7], (uint32_t)args[8], (uint32_t)args[9], (uint32_t)args[10], 0u, 0u};
        if (const char *why = conv_shape_check(cs)) return fail(COFHE_HIP_EINVAL, why);
        p = plan_conv2d(cs, (uint32_t)args[11], (uint32_t)args[12]);
    } else if (o == "conv2d_grouped" && need(16)) {
        // B, H, W, C, kh, kw, Co, sh, sw, ph, pw, dh, dw, groups, exp_bits, w: the direct route of
        // cofhe_hip_conv2d_grouped_plain_ct_records
        for (int i = 0; i < 16; i++)
            if (args[i] > 0xFFFFFFFFull) return fail(COFHE_HIP_EINVAL, "conv2d_grouped plan: argument out of range");
        if (args[15] < 2 || args[15] > 8) return fail(COFHE_HIP_EINVAL, "conv2d_grouped plan: w in 2..8");
        ConvShape cs{(uint32_t)args[0], (uint32_t)args[1], (uint32_t)args[2], (uint32_t)args[3], (uint32_t)args[4], (uint32_t)args[5], (uint32_t)args[6],
                     (uint32_t)args[7], (uint32_t)args[8], (uint32_t)args[9], (uint32_t)args[10], 0u, 0u,
                     (uint32_t)args[11], (uint32_t)args[12], (uint32_t)args[13]};
        if (const char *why = conv_shape_check(cs)) return fail(COFHE_HIP_EINVAL, why);
        p = plan_conv2d(cs, (uint32_t)args[14], (uint32_t)args[15]);
    } else if (o == "accumulate_tree" && need(3)) {
        p = plan_accumulate_tree((uint32_t)args[0], (uint32_t)args[1], (uint32_t)args[2]);
    } else if (o == "encrypt_chunk" && need(2)) {
        p = plan_encrypt_chunk(args[0], (uint32_t)args[1]);
    } else if (o == "fixed_base" && need(2)) {
        p = plan_fixed_base((uint32_t)args[0], (uint32_t)args[1]);
    } else if (o == "comb" && need(6)) {
        // kind (0..4), n items, exp_bits, kbits, w (0: automatic), chunk (0: automatic): the regions of one (the largest) chunk
        if (int rc = comb_check(args[0], args[1], args[2], args[3], args[4], args[5])) return rc;
        const CombCall cc = comb_call((uint32_t)args[0], args[1], (uint32_t)args[2], (uint32_t)args[3], (uint32_t)args[4], args[5]);
        p = plan_comb_chunk(cc.s, cc.chunk);
    } else {
        return fail(COFHE_HIP_EINVAL, "unknown workspace plan or wrong argument count: " + o);
    }
    *n_regions = (uint32_t)p.n;
    *total_bytes = p.total;
    for (int i = 0; i < p.n && (uint32_t)i < cap && regions; i++) regions[i] = p.r[i];
    return COFHE_HIP_OK;
}

namespace {
struct StreamTimer {
    hipEvent_t a = nullptr, b = nullptr;
};
}  // namespace
int cofhe_hip_timer_start(cofhe_hip_ctx *ctx, void *stream, void **timer) {
    if (!ctx || !timer) return fail(COFHE_HIP_EINVAL, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    StreamTimer *t = new StreamTimer();
    hipError_t e = hipEventCreate(&t->a);
    if (e == hipSuccess) e = hipEventCreate(&t->b);
    if (e == hipSuccess) e = hipEventRecord(t->a, (hipStream_t)stream);
    if (e != hipSuccess) {
        if (t->a) (void)hipEventDestroy(t->a);
        if (t->b) (void)hipEventDestroy(t->b);
        delete t;
        return fail(COFHE_HIP_EHIP, std::string("stream timer: ") + hipGetErrorString(e));
    }
    *timer = t;
    return COFHE_HIP_OK;
}
int cofhe_hip_timer_stop(cofhe_hip_ctx *ctx, void *timer, void *stream, float *ms) {
    if (!ctx || !timer || !ms) return fail(COFHE_HIP_EINVAL, "null argument");
    StreamTimer *t = (StreamTimer *)timer;
    hipError_t e = hipEventRecord(t->b, (hipStream_t)stream);
    if (e == hipSuccess) e = hipEventSynchronize(t->b);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, t->a, t->b);
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
    if (e != hipSuccess) return fail(COFHE_HIP_EHIP, std::string("stream timer: ") + hipGetErrorString(e));
    return COFHE_HIP_OK;
}

// ---- formats ---------------------------------------------------------------------------------
namespace {
// little-endian byte strings <-> limb records
struct IntView {
    const uint8_t *p;
    size_t n;
    bool neg;
};

int parse_tensor(const uint8_t *bytes, size_t len, size_t per_elem, uint32_t *ndim, uint32_t shape[8],
                 std::vector<IntView> &ints) {
    if (len < 4) return fail(COFHE_HIP_EINVAL, "tensor buffer too short");
    uint32_t nd;
    memcpy(&nd, bytes, 4);
    if (nd > 8) return fail(COFHE_HIP_EINVAL, "tensor rank above 8");
    if (len < 4 + 4ull * nd) return fail(COFHE_HIP_EINVAL, "tensor buffer too short");
    uint64_t ne = 1;
    for (uint32_t i = 0; i < nd; i++) {
        memcpy(&shape[i], bytes + 4 + 4 * i, 4);
        if (shape[i] != 0 && ne > (1ull << 40) / shape[i]) return fail(COFHE_HIP_EINVAL, "tensor too large");     // before the product can wrap
        ne *= shape[i];
    }
    *ndim = nd;
    const uint64_t cnt = ne * per_elem;
    const size_t hdr = 4 + 4ull * nd + 8ull * cnt;
    if (len < hdr) return fail(COFHE_HIP_EINVAL, "tensor buffer too short");
    const uint8_t *tab = bytes + 4 + 4ull * nd;
    const uint8_t *body = bytes + hdr;
    const size_t blen = len - hdr;
    ints.resize(cnt);
    const uint64_t M = ~(1ull << 63);
    for (uint64_t i = 0; i < cnt; i++) {
        uint64_t o, o2;
        memcpy(&o, tab + 8 * i, 8);
        if (i + 1 < cnt) {
            memcpy(&o2, tab + 8 * (i + 1), 8);
            o2 &= M;
        } else {
            o2 = blen;
        }
        const uint64_t st = o & M;
        if (o2 < st || o2 > blen) return fail(COFHE_HIP_EINVAL, "corrupt offset table");
        ints[i] = IntView{body + st, (size_t)(o2 - st), (o >> 63) != 0};
    }
    return COFHE_HIP_OK;
}

bool put_limbs(uint32_t *dst, int words, const IntView &v) {
    size_t n = sig_bytes(v.p, v.n);
    if (n > (size_t)words * 4) return false;
    memset(dst, 0, (size_t)words * 4);
    memcpy(dst, v.p, n);     // little-endian host
    return true;
}

// forms_per_elem = 2: ciphertext tensors (c1, c2); 1: partial-decryption tensors (one form each)
int form_bytes_to_records(const uint8_t *bytes, size_t len, int forms_per_elem, uint32_t *ndim, uint32_t shape[8],
                          uint32_t **records, uint64_t *n_records) {
    std::vector<IntView> ints;
    if (int rc = parse_tensor(bytes, len, 3 * (size_t)forms_per_elem, ndim, shape, ints)) return rc;
    const uint64_t nrec = ints.size() / 3;
    uint32_t *r = (uint32_t *)calloc(nrec ? nrec * REC_WORDS : 1, 4);
    if (!r) return fail(COFHE_HIP_ENOMEM, "out of host memory");
    for (uint64_t i = 0; i < nrec; i++) {
        uint32_t *rec = r + i * REC_WORDS;
        const IntView &a = ints[3 * i], &b = ints[3 * i + 1], &cc = ints[3 * i + 2];
        bool ok = put_limbs(rec + REC_A, PLIMBS, a) && put_limbs(rec + REC_B, PLIMBS, b) &&
                  put_limbs(rec + REC_C, 2 * PLIMBS, cc);
        // a and c of a form are positive: zero is refused, and so is the flag on a non-zero a or c, which the reference's
        // reader would negate (a flagged zero is refused as zero)
        if (ok && (bits_of(rec + REC_A, PLIMBS) == 0 || bits_of(rec + REC_C, 2 * PLIMBS) == 0)) ok = false;
        if (ok && (a.neg || cc.neg)) ok = false;
        if (!ok) {
            free(r);
            return fail(COFHE_HIP_EINVAL, "form coefficient outside the supported range");
        }
        rec[REC_SIGN] = (b.neg && bits_of(rec + REC_B, PLIMBS) != 0) ? 1u : 0u;
    }
    *records = r;
    *n_records = nrec;
    return COFHE_HIP_OK;
}

int form_records_to_bytes(const uint32_t *records, uint64_t nrec, int forms_per_elem, uint32_t ndim,
                          const uint32_t *shape, uint8_t **bytes, size_t *len) {
    uint64_t ne = 1;
    for (uint32_t i = 0; i < ndim; i++) {
        if (shape[i] != 0 && ne > (1ull << 40) / shape[i]) return fail(COFHE_HIP_EINVAL, "tensor too large");
        ne *= shape[i];
    }
    if (ne * (uint64_t)forms_per_elem != nrec) return fail(COFHE_HIP_EINVAL, "shape does not match the record count");
    const uint64_t cnt = nrec * 3;
    std::vector<uint64_t> offs(cnt);
    uint64_t last = 0;
    for (uint64_t i = 0; i < nrec; i++) {
        const uint32_t *rec = records + i * REC_WORDS;
        const size_t ba = bits_of(rec + REC_A, PLIMBS), bb = bits_of(rec + REC_B, PLIMBS),
                     bc = bits_of(rec + REC_C, 2 * PLIMBS);
        // slot width = mpz_sizeinbase(x, 2) / 8 + 1 (sizeinbase(0) == 1); flag = (sgn != 1)
        const size_t w[3] = {(ba ? ba : 1) / 8 + 1, (bb ? bb : 1) / 8 + 1, (bc ? bc : 1) / 8 + 1};
        const bool flag[3] = {ba == 0, bb == 0 || rec[REC_SIGN] != 0, bc == 0};
        for (int k = 0; k < 3; k++) {
            offs[3 * i + k] = last | (flag[k] ? (1ull << 63) : 0ull);
            last += w[k];
        }
    }
    const size_t hdr = 4 + 4ull * ndim + 8ull * cnt;
    const size_t total = hdr + last;
    uint8_t *out = (uint8_t *)calloc(total ? total : 1, 1);
    if (!out) return fail(COFHE_HIP_ENOMEM, "out of host memory");
    memcpy(out, &ndim, 4);
    for (uint32_t i = 0; i < ndim; i++) memcpy(out + 4 + 4 * i, &shape[i], 4);
    memcpy(out + 4 + 4ull * ndim, offs.data(), 8ull * cnt);
    uint8_t *body = out + hdr;
    const uint64_t M = ~(1ull << 63);
    for (uint64_t i = 0; i < nrec; i++) {
        const uint32_t *rec = records + i * REC_WORDS;
        const uint32_t *src[3] = {rec + REC_A, rec + REC_B, rec + REC_C};
        for (int k = 0; k < 3; k++) {
            const uint64_t st = offs[3 * i + k] & M;
            const uint64_t en = (3 * i + k + 1 < cnt) ? (offs[3 * i + k + 1] & M) : last;
            memcpy(body + st, src[k], (size_t)(en - st));   // slot never exceeds the limb array
        }
    }
    *bytes = out;
    *len = total;
    return COFHE_HIP_OK;
}

}  // namespace

int cofhe_hip_bytes_to_records(const uint8_t *bytes, size_t len, uint32_t *ndim, uint32_t shape[8], uint32_t **records,
                               uint64_t *n_records) {
    return form_bytes_to_records(bytes, len, 2, ndim, shape, records, n_records);
}
int cofhe_hip_records_to_bytes(const uint32_t *records, uint64_t nrec, uint32_t ndim, const uint32_t *shape,
                               uint8_t **bytes, size_t *len) {
    return form_records_to_bytes(records, nrec, 2, ndim, shape, bytes, len);
}
int cofhe_hip_pdr_bytes_to_records(const uint8_t *bytes, size_t len, uint32_t *ndim, uint32_t shape[8],
                                   uint32_t **records, uint64_t *n_records) {
    return form_bytes_to_records(bytes, len, 1, ndim, shape, records, n_records);
}
int cofhe_hip_pdr_records_to_bytes(const uint32_t *records, uint64_t nrec, uint32_t ndim, const uint32_t *shape,
                                   uint8_t **bytes, size_t *len) {
    return form_records_to_bytes(records, nrec, 1, ndim, shape, bytes, len);
}

int cofhe_hip_bytes_to_exponents(const uint8_t *bytes, size_t len, uint32_t *ndim, uint32_t shape[8], uint32_t **exps,
                                 uint64_t *n_exps) {
    std::vector<IntView> ints;
    if (int rc = parse_tensor(bytes, len, 1, ndim, shape, ints)) return rc;
    uint32_t *r = (uint32_t *)calloc(ints.size() ? ints.size() * EXP_REC_WORDS : 1, 4);
    if (!r) return fail(COFHE_HIP_ENOMEM, "out of host memory");
    for (size_t i = 0; i < ints.size(); i++) {
        uint32_t *rec = r + i * EXP_REC_WORDS;
        if (!put_limbs(rec, EXP_MAG_WORDS, ints[i])) {
            free(r);
            return fail(COFHE_HIP_EINVAL, "exponent wider than 992 bits");
        }
        rec[EXP_MAG_WORDS] = (ints[i].neg && bits_of(rec, EXP_MAG_WORDS) != 0) ? 1u : 0u;
    }
    *exps = r;
    *n_exps = ints.size();
    return COFHE_HIP_OK;
}

// ---- whole operations on host buffers ---------------------------------------------------------
// The serialised tensors are uploaded verbatim and converted on the GPU (wire.hip): PCIe carries the
// ~786 B/ciphertext of the wire format instead of 1344 B of records, and no host loop touches the data.
namespace {
// host bytes -> device records; kind as in cofhe_hip_unpack_tensor_device
int load_tensor(cofhe_hip_ctx *ctx, const uint8_t *bytes, size_t len, int kind, DevBuf &recs, uint32_t *ndim,
                uint32_t shape[8], uint64_t *n_records) {
    if (len < 4) return fail(COFHE_HIP_EINVAL, "tensor buffer too short");
    const size_t rec_bytes = kind == 0 ? EXP_REC_WORDS * 4 : REC_WORDS * 4;
    const uint64_t cap = (len / 8) / (kind == 0 ? 1 : 3) + 1;      // every integer owns an 8-byte table entry
    DevBuf raw;
    if (int rc = raw.get(ctx, len)) return rc;
    if (int rc = recs.get(ctx, cap * rec_bytes)) return rc;
    HIPCHK(hipMemcpy(raw.p, bytes, len, hipMemcpyHostToDevice));
    return cofhe_hip_unpack_tensor_device(ctx, raw.p, len, kind, recs.p, cap, ndim, shape, n_records, nullptr);
}
int finish(cofhe_hip_ctx *ctx, const DevBuf &dout, uint64_t nrec, uint32_t ndim, const uint32_t *shape, uint8_t **out,
           size_t *outlen) {
    const size_t cap = cofhe_hip_packed_size_bound(nrec, 2, ndim);
    DevBuf packed;
    if (int rc = packed.get(ctx, cap)) return rc;
    size_t len = 0;
    if (int rc = cofhe_hip_pack_tensor_device(ctx, dout.p, nrec, 2, ndim, shape, packed.p, cap, &len, nullptr)) return rc;
    uint8_t *h = (uint8_t *)malloc(len ? len : 1);
    if (!h) return fail(COFHE_HIP_ENOMEM, "out of host memory");
    hipError_t e = hipMemcpy(h, packed.p, len, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        free(h);
        return fail(COFHE_HIP_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    *out = h;
    *outlen = len;
    return COFHE_HIP_OK;
}
// two ciphertext tensors of equal shape through one of the ciphertext-pair entry points
int ct_pair_bytes(cofhe_hip_ctx *ctx, int (*op)(cofhe_hip_ctx *, const void *, const void *, void *, uint64_t, void *), const uint8_t *t1, size_t l1,
                  const uint8_t *t2, size_t l2, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    uint32_t nd1, nd2, s1[8], s2[8];
    uint64_t n1, n2;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf da, db, dc;
    if (int rc = load_tensor(ctx, t1, l1, 2, da, &nd1, s1, &n1)) return rc;
    if (int rc = load_tensor(ctx, t2, l2, 2, db, &nd2, s2, &n2)) return rc;
    if (nd1 != nd2 || memcmp(s1, s2, 4 * nd1) != 0) return fail(COFHE_HIP_ESHAPE, "Tensor shapes must be equal");
    const size_t bytes = (size_t)n1 * REC_WORDS * 4;
    if (int rc = dc.get(ctx, bytes ? bytes : 4)) return rc;
    if (int rc = op(ctx, da.p, db.p, dc.p, n1 / 2, nullptr)) return rc;
    return finish(ctx, dc, n1, nd1, s1, out, outlen);
}
}  // namespace

int cofhe_hip_add_ciphertext_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *t1, size_t l1, const uint8_t *t2, size_t l2,
                                           uint8_t **out, size_t *outlen) {
    return ct_pair_bytes(ctx, cofhe_hip_add_ciphertext_records, t1, l1, t2, l2, out, outlen);
}
int cofhe_hip_sub_ciphertext_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *t1, size_t l1, const uint8_t *t2, size_t l2,
                                           uint8_t **out, size_t *outlen) {
    return ct_pair_bytes(ctx, cofhe_hip_sub_ciphertext_records, t1, l1, t2, l2, out, outlen);
}
int cofhe_hip_add_plaintext_tensor_bytes(cofhe_hip_ctx *ctx, const uint8_t *cts, size_t lc, const uint8_t *pt, size_t lp,
                                         const uint32_t *f_record, uint32_t kbits, int mode, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (mode < 0 || mode > 2) return fail(COFHE_HIP_EINVAL, "add_plain: mode 0 (ct + m), 1 (ct - m) or 2 (m - ct)");
    uint32_t ndc, ndp, sc[8], sp[8];
    uint64_t nr, ne;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf dc, dp;
    if (int rc = load_tensor(ctx, cts, lc, 2, dc, &ndc, sc, &nr)) return rc;
    if (int rc = load_tensor(ctx, pt, lp, 0, dp, &ndp, sp, &ne)) return rc;
    if (ndc != ndp || memcmp(sc, sp, 4 * ndc) != 0 || nr != 2 * ne) return fail(COFHE_HIP_ESHAPE, "Tensor shapes must be equal");
    if (int rc = cofhe_hip_add_plain_records(ctx, dc.p, dp.p, nullptr, nullptr, nullptr, f_record, dc.p, ne, kbits, mode, nullptr)) return rc;
    return finish(ctx, dc, nr, ndc, sc, out, outlen);
}

int cofhe_hip_scal_ciphertext_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *s, size_t ls, const uint8_t *cts, size_t lc,
                                            const uint8_t *zero, size_t lz, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    uint32_t nds, ndc, ss[8], sc[8];
    uint64_t ne, nr;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf de, dc, dz, dout;
    if (int rc = load_tensor(ctx, s, ls, 0, de, &nds, ss, &ne)) return rc;
    if (int rc = load_tensor(ctx, cts, lc, 2, dc, &ndc, sc, &nr)) return rc;
    if (nds > 2 || ndc > 2 || nds != ndc)
        return fail(COFHE_HIP_ENDIM, "Tensors must be 0D, 1D or 2D for now");
    if (nds <= 1) {
        // 0-D x 0-D (one exponent, one ciphertext: tensor_ops.inl:275-278, without the reference's re-randomisation --
        // this entry point is deterministic) and 1-D x 1-D element-wise
        if (nds == 1 && ss[0] != sc[0]) return fail(COFHE_HIP_ESHAPE, "Vector sizes must be equal");
        if (ne * 2 != nr) return fail(COFHE_HIP_ESHAPE, "Vector sizes must be equal");
        if (int rc = dout.get(ctx, nr ? nr * REC_WORDS * 4 : 4)) return rc;
        if (int rc = cofhe_hip_pow_records(ctx, dc.p, de.p, dout.p, nr / 2, nullptr)) return rc;
        return finish(ctx, dout, nr, ndc, sc, out, outlen);
    }
    // 2-D: cts n x m, s m x p
    const uint32_t n = sc[0], m = sc[1], p = ss[1];
    if (ss[0] != m) return fail(COFHE_HIP_ESHAPE, "inner dimensions of the matrix product differ");
    uint32_t ndz, sz[8];
    uint64_t nz;
    if (!zero) return fail(COFHE_HIP_EINVAL, "the 2-D product needs the encryption of zero it starts from");
    if (int rc = load_tensor(ctx, zero, lz, 2, dz, &ndz, sz, &nz)) return rc;
    if (nz != 2) return fail(COFHE_HIP_EINVAL, "zero must be a one-element ciphertext tensor");
    const uint64_t nout = (uint64_t)n * p * 2;
    if (int rc = dout.get(ctx, nout ? nout * REC_WORDS * 4 : 4)) return rc;
    if (int rc = cofhe_hip_scal_matmul_records(ctx, dc.p, de.p, dz.p, dout.p, n, m, p, nullptr)) return rc;
    const uint32_t so[2] = {n, p};
    return finish(ctx, dout, nout, 2, so, out, outlen);
}

int cofhe_hip_matmul_plain_ct_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *s, size_t ls, const uint8_t *cts, size_t lc,
                                            const uint8_t *zero, size_t lz, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    uint32_t nds, ndc, ss[8], sc[8];
    uint64_t ne, nr;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf de, dc, dz, dout;
    if (int rc = load_tensor(ctx, s, ls, 0, de, &nds, ss, &ne)) return rc;
    if (int rc = load_tensor(ctx, cts, lc, 2, dc, &ndc, sc, &nr)) return rc;
    if (nds != 2 || ndc != 2) return fail(COFHE_HIP_ESHAPE, "the plaintext-left product takes two matrices");
    // s n x m, cts m x p
    const uint32_t n = ss[0], m = ss[1], p = sc[1];
    if (sc[0] != m) return fail(COFHE_HIP_ESHAPE, "inner dimensions of the matrix product differ");
    uint32_t ndz, sz[8];
    uint64_t nz;
    if (!zero) return fail(COFHE_HIP_EINVAL, "the 2-D product needs the encryption of zero it starts from");
    if (int rc = load_tensor(ctx, zero, lz, 2, dz, &ndz, sz, &nz)) return rc;
    if (nz != 2) return fail(COFHE_HIP_EINVAL, "zero must be a one-element ciphertext tensor");
    const uint64_t nout = (uint64_t)n * p * 2;
    if (int rc = dout.get(ctx, nout ? nout * REC_WORDS * 4 : 4)) return rc;
    if (int rc = cofhe_hip_matmul_plain_ct_records(ctx, de.p, dc.p, dz.p, dout.p, n, m, p, nullptr)) return rc;
    const uint32_t so[2] = {n, p};
    return finish(ctx, dout, nout, 2, so, out, outlen);
}

namespace {
// the serialised twin of conv2d_run: w null = sum pooling over kh x kw windows (no filter tensor; Co = groups = C)
int conv2d_bytes(cofhe_hip_ctx *ctx, const uint8_t *w, size_t lw, const uint8_t *cts, size_t lc, const uint8_t *zero, size_t lz,
                 cofhe_hip_conv2d_geometry g, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    uint32_t ndw = 0, ndc, swp[8], sc[8];
    uint64_t ne, nr;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf de, dc, dz, dout;
    if (w)
        if (int rc = load_tensor(ctx, w, lw, 0, de, &ndw, swp, &ne)) return rc;
    if (int rc = load_tensor(ctx, cts, lc, 2, dc, &ndc, sc, &nr)) return rc;
    if (w && (ndw != 4 || ndc != 4))
        return fail(COFHE_HIP_ESHAPE, "conv2d takes a 4-D filter tensor [kh, kw, C / groups, Co] and a 4-D image tensor [B, H, W, C]");
    if (!w && ndc != 4) return fail(COFHE_HIP_ESHAPE, "sum_pool2d takes a 4-D image tensor [B, H, W, C]");
    g.B = sc[0], g.H = sc[1], g.W = sc[2], g.C = sc[3];
    if (w) {
        g.kh = swp[0], g.kw = swp[1], g.Co = swp[3];
        if (g.groups && swp[2] != g.C / g.groups) return fail(COFHE_HIP_ESHAPE, "conv2d: the channels of the filters and of the image differ");
    } else {
        g.Co = g.C;
        g.groups = g.C ? g.C : 1;
    }
    uint32_t Ho = 0, Wo = 0;
    if (int rc = cofhe_hip_conv2d_geometry_out_shape(&g, &Ho, &Wo)) return rc;
    uint32_t ndz, sz[8];
    uint64_t nz;
    if (!zero) return fail(COFHE_HIP_EINVAL, "conv2d needs the encryption of zero it starts from");
    if (int rc = load_tensor(ctx, zero, lz, 2, dz, &ndz, sz, &nz)) return rc;
    if (nz != 2) return fail(COFHE_HIP_EINVAL, "zero must be a one-element ciphertext tensor");
    const uint32_t so[4] = {g.B, Ho, Wo, g.Co};
    const uint64_t nout = (uint64_t)so[0] * Ho * Wo * so[3] * 2;
    if (int rc = dout.get(ctx, nout ? nout * REC_WORDS * 4 : 4)) return rc;
    if (w) {
        if (int rc = cofhe_hip_conv2d_grouped_plain_ct_records(ctx, de.p, dc.p, dz.p, dout.p, &g, nullptr)) return rc;
    } else {
        if (int rc = cofhe_hip_sum_pool2d_records(ctx, dc.p, dz.p, dout.p, &g, nullptr)) return rc;
    }
    return finish(ctx, dout, nout, 4, so, out, outlen);
}
}  // namespace

int cofhe_hip_conv2d_plain_ct_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *w, size_t lw, const uint8_t *cts, size_t lc, const uint8_t *zero,
                                            size_t lz, uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw, uint8_t **out, size_t *outlen) {
    if (!w) return fail(COFHE_HIP_EINVAL, "null argument");
    // dh = dw = groups = 1: conv2d_run then launches what cofhe_hip_conv2d_plain_ct_records launches
    return conv2d_bytes(ctx, w, lw, cts, lc, zero, lz, cofhe_hip_conv2d_geometry{0, 0, 0, 0, 0, 0, 0, sh, sw, ph, pw, 1, 1, 1}, out, outlen);
}
int cofhe_hip_conv2d_grouped_plain_ct_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *w, size_t lw, const uint8_t *cts, size_t lc,
                                                    const uint8_t *zero, size_t lz, uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw,
                                                    uint32_t dh, uint32_t dw, uint32_t groups, uint8_t **out, size_t *outlen) {
    if (!w) return fail(COFHE_HIP_EINVAL, "null argument");
    return conv2d_bytes(ctx, w, lw, cts, lc, zero, lz, cofhe_hip_conv2d_geometry{0, 0, 0, 0, 0, 0, 0, sh, sw, ph, pw, dh, dw, groups}, out, outlen);
}
int cofhe_hip_sum_pool2d_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *cts, size_t lc, const uint8_t *zero, size_t lz, uint32_t kh, uint32_t kw,
                                       uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw, uint8_t **out, size_t *outlen) {
    return conv2d_bytes(ctx, nullptr, 0, cts, lc, zero, lz, cofhe_hip_conv2d_geometry{0, 0, 0, 0, kh, kw, 0, sh, sw, ph, pw, 1, 1, 1}, out, outlen);
}

int cofhe_hip_poly_close_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *coef, size_t lcoef, const uint8_t *e, size_t le, const uint8_t *powers,
                                       size_t lp, const uint32_t *f_record, uint32_t kbits, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    uint32_t ndk, nde, ndp, sk[8], se[8], sp[8];
    uint64_t nk, ne, nr;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf dk, de, dp, dout;
    if (int rc = load_tensor(ctx, coef, lcoef, 0, dk, &ndk, sk, &nk)) return rc;
    if (int rc = load_tensor(ctx, e, le, 0, de, &nde, se, &ne)) return rc;
    if (int rc = load_tensor(ctx, powers, lp, 2, dp, &ndp, sp, &nr)) return rc;
    if (ndk != 1 || nk < 2 || nk > (uint64_t)POLY_MAX_DEGREE + 1)
        return fail(COFHE_HIP_ESHAPE, "poly_close: the coefficients are a 1-D plaintext tensor of 2 to 9 elements");
    const uint32_t d = (uint32_t)nk - 1;
    if (ndp != nde + 1 || sp[0] != d || memcmp(sp + 1, se, 4 * nde) != 0 || nr != 2 * ne * d)
        return fail(COFHE_HIP_ESHAPE, "poly_close: the powers are a ciphertext tensor [d, shape of e]");
    if (int rc = dout.get(ctx, ne ? ne * 2 * REC_WORDS * 4 : 4)) return rc;
    if (int rc = cofhe_hip_poly_close_records(ctx, dk.p, de.p, dp.p, f_record, dout.p, ne, d, kbits, nullptr)) return rc;
    return finish(ctx, dout, 2 * ne, nde, se, out, outlen);
}

int cofhe_hip_div_close_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *e, size_t le, const uint8_t *div, size_t ldiv, const uint8_t *rq,
                                      size_t lrq, const uint32_t *f_record, uint32_t kbits, uint8_t **out, size_t *outlen) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!k_in_range(kbits)) return fail(COFHE_HIP_EINVAL, "k out of range");
    // the divisors are public host values: read and judged here, as the kernel judges them
    uint32_t ndd, sd[8], *hdiv = nullptr;
    uint64_t nd;
    if (int rc = cofhe_hip_bytes_to_exponents(div, ldiv, &ndd, sd, &hdiv, &nd)) return rc;
    struct Free {
        uint32_t *p;
        ~Free() { free(p); }
    } guard{hdiv};
    const int L = pmm_limbs(kbits);
    for (uint64_t i = 0; i < nd; i++) {
        const uint32_t *rec = hdiv + i * EXP_REC_WORDS;
        uint32_t any = 0;
        for (int l = 0; l < L; l++) any |= l == L - 1 ? rec[l] & pmm_top_mask(kbits) : rec[l];
        if (rec[EXP_MAG_WORDS] != 0 || any == 0 || ((rec[(kbits - 1) >> 5] >> ((kbits - 1) & 31)) & 1u))
            return fail(COFHE_HIP_EINVAL, "div_close: a divisor D needs 1 <= D < 2^(k-1)");
    }
    uint32_t nde, ndr, se[8], sr[8];
    uint64_t ne, nr;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf de, dd, dr, dout;
    if (int rc = load_tensor(ctx, e, le, 0, de, &nde, se, &ne)) return rc;
    if (int rc = load_tensor(ctx, rq, lrq, 2, dr, &ndr, sr, &nr)) return rc;
    if (ndr != nde || memcmp(sr, se, 4 * nde) != 0 || nr != 2 * ne)
        return fail(COFHE_HIP_ESHAPE, "div_close: [r_q] is a ciphertext tensor of e's shape");
    // one divisor, one per channel (the last dimension of e) or one per element
    const bool per_channel = nde >= 1 && ndd == 1 && sd[0] == se[nde - 1];
    const bool per_element = ndd == nde && memcmp(sd, se, 4 * nde) == 0;
    if (nd == 0 || !(nd == 1 || per_channel || per_element))
        return fail(COFHE_HIP_ESHAPE, "div_close: the divisors are one element, e's last dimension or e's shape");
    if (int rc = dd.get(ctx, nd * EXP_REC_WORDS * 4)) return rc;
    HIPCHK(hipMemcpy(dd.p, hdiv, nd * EXP_REC_WORDS * 4, hipMemcpyHostToDevice));
    if (int rc = dout.get(ctx, ne ? ne * 2 * REC_WORDS * 4 : 4)) return rc;
    if (int rc = cofhe_hip_div_close_records(ctx, de.p, dd.p, nd, dr.p, f_record, dout.p, ne, kbits, nullptr)) return rc;
    return finish(ctx, dout, 2 * ne, nde, se, out, outlen);
}

}  // extern "C"
