// prims_gpu.hip -- TEST INFRASTRUCTURE: the device arithmetic primitives (cofhe_amd/csrc/lane.hpp, mp.hpp, wide.hpp, and the
// remainder sequences built on them) run ON THE GPU one primitive at a time, against Python integers
// (tests/test_gpu_prims.py).  The host simulators (tests/hostsim) replace exactly what is most likely to be wrong on the
// device: the DPP / ds_bpermute / ballot cross-lane primitives, the inline-asm carry chain of lincomb_plane, the wide layout's
// wave shifts and readlanes, and any_lane, which on the device is a ballot over the WHOLE wavefront -- a group enters guarded
// code because a neighbouring group needs it.  Here those are the real instructions.
//
// Throughput layout: 64 threads per workgroup, one instance per 8-lane group, the context set up as the kernels do it
// (wg_ctx.hpp: make_served_ctx); every launch takes a map slot_active[n_groups], and the groups it switches off return at
// once, so a wavefront runs with any subset of its eight groups live (the partial-EXEC case lane.hpp promises is well
// defined).  Record layout per group: packed limbs as in tests/hostsim/sim.cpp (ld / st), so tests/simlib.py's pack / unpack
// serve both tiers; group g reads in + g * IN words and writes out + g * OUT words (prims_gpu_words).
// Wide layout: one number per wavefront, one or four wavefronts per workgroup.
//
// The headers are inlined into these small kernels, so register allocation and scheduling differ from the product's
// kernels: this proves the source-level routes, not the product's code object.
// Built by __graft_entry__.build() into tests/gpu_kernels/libprims_gpu.so.  Not part of the product.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../cofhe_amd/csrc/form_io.hpp"
#include "../../cofhe_amd/csrc/qfw.hpp"
#include "../../cofhe_amd/csrc/wg_ctx.hpp"
#include "../../cofhe_amd/csrc/wide.hpp"

using namespace cofhe;

namespace {

template <int P>
__device__ Mp<P> ld(const Ctx &c, const uint32_t *w) {
    Mp<P> x;
    CF_UNROLL for (int p = 0; p < P; p++)
        CF_UNROLL for (int j = 0; j < CH; j++) x.v[p][j] = w[p * PLIMBS + c.gl * CH + j];
    return x;
}
template <int P>
__device__ void st(const Ctx &c, const Mp<P> &x, uint32_t *w) {
    CF_UNROLL for (int p = 0; p < P; p++)
        CF_UNROLL for (int j = 0; j < CH; j++) w[p * PLIMBS + c.gl * CH + j] = x.v[p][j];
}

// ---------------------------------------------------------------------------- throughput layout: one op per kernel
enum Op { OP_LANE, OP_MUL11, OP_MUL21, OP_LINCOMB, OP_SHIFT, OP_BITS, OP_DIVREM21, OP_DIVREM11, OP_DIVREM22, OP_WORD, OP_PRIMORIAL,
          OP_DIVEXACT, OP_XGCD, OP_COUNT };
constexpr int LANE_OUT = 18;        // words per lane of OP_LANE
// words per group: input, output
constexpr int OP_WORDS[OP_COUNT][2] = {
    {2 * G, LANE_OUT * G},          // LANE: per lane (value, predicate) -> LANE_OUT results per lane
    {80, 80},                       // MUL11: x[40] y[40] -> x y
    {120, 120},                     // MUL21: x[80] y[40] -> x y
    {162, 243},                     // LINCOMB: x[80] y[80] A B -> A x - B y [80] | A x + B y [80] | x + y [80] | word of the difference, of the sum, carry of x + y
    {81, 241},                      // SHIFT: x[80] n -> x << n | x >> n | x >> 1 | bit length
    {162, 5},                       // BITS: x[80] y[80] pos idx -> cmp | bits64 low, high | bits32 | limb idx
    {120, 160},                     // DIVREM21: num[80] den[40] -> quot[80] rem[80]
    {80, 80},                       // DIVREM11: num[40] den[40] -> quot[40] rem[40]
    {160, 160},                     // DIVREM22: num[80] den[80] -> quot[80] rem[80]
    {81, 84},                       // WORD: x[80] W -> x / W [80] | x mod W (mp_divrem_word) | mp_mod_word | mp_mod_word_fast of plane 0, of x
    {40, 1},                        // PRIMORIAL: x[40] -> x mod 223092870
    {121, 80},                      // DIVEXACT: num[80] den[40] nq -> quot[80]
    {80, 81},                       // XGCD: x[40] y[40] -> gcd[40] u[40] sign
};

template <int OP>
__device__ void run_op(Ctx &c, const uint32_t *in, uint32_t *out) {
    if constexpr (OP == OP_LANE) {
        const uint32_t v = in[2 * c.gl];
        const bool p = in[2 * c.gl + 1] != 0;
        uint32_t *o = out + LANE_OUT * c.gl;
        uint32_t r[LANE_OUT];
        CF_UNROLL for (int s = 0; s < G; s++) r[s] = s & 1 ? bcast(c, v, s) : shfl(c, v, s);
        r[8] = shfl_up1(c, v, ~v);
        r[9] = shfl_down1(c, v, ~v);
        r[10] = shfl_xor1(c, v);
        r[11] = shfl_xor2(c, v);
        r[12] = shfl_mirror(c, v);
        r[13] = bcast_first(c, v);
        r[14] = bcast_last(c, v);
        r[15] = ballot8(c, p);
        r[16] = any_lane(c, p) ? 1u : 0u;
        r[17] = group_max(c, v);
        for (int k = 0; k < LANE_OUT; k++) o[k] = r[k];
    } else if constexpr (OP == OP_MUL11) {
        st(c, mp_mul(c, ld<1>(c, in), ld<1>(c, in + 40)), out);
    } else if constexpr (OP == OP_MUL21) {
        st(c, mp_mul(c, ld<2>(c, in), ld<1>(c, in + 80)), out);
    } else if constexpr (OP == OP_LINCOMB) {
        const Mp<2> a = ld<2>(c, in), b = ld<2>(c, in + 80);
        const uint32_t A = in[160], B = in[161];
        Mp<2> o;
        const uint32_t ws = mp_lincomb_sub_carry(c, o, A, a, B, b);
        st(c, o, out);
        const uint32_t wa = mp_lincomb_add(c, o, A, a, B, b);
        st(c, o, out + 80);
        const uint32_t cy = mp_add(c, o, a, b);
        st(c, o, out + 160);
        if (c.gl == 0) {
            out[240] = ws;
            out[241] = wa;
            out[242] = cy;
        }
    } else if constexpr (OP == OP_SHIFT) {
        const Mp<2> a = ld<2>(c, in);
        const int n = (int)in[80];
        st(c, mp_shl(c, a, n), out);
        st(c, mp_shr(c, a, n), out + 80);
        st(c, mp_shr1(c, a), out + 160);
        const int b = mp_bitlen(c, a);
        if (c.gl == 0) out[240] = (uint32_t)b;
    } else if constexpr (OP == OP_BITS) {
        const Mp<2> a = ld<2>(c, in), b = ld<2>(c, in + 80);
        const int pos = (int)in[160], idx = (int)in[161];
        const int cm = mp_cmp(c, a, b);
        const uint64_t w = mp_bits64(c, a, pos);
        const uint32_t h = mp_bits32(c, a, pos), l = mp_get_limb(c, a, idx);
        if (c.gl == 0) {
            out[0] = (uint32_t)cm;
            out[1] = (uint32_t)w;
            out[2] = (uint32_t)(w >> 32);
            out[3] = h;
            out[4] = l;
        }
    } else if constexpr (OP == OP_DIVREM21) {
        Mp<2> n = ld<2>(c, in), q;
        mp_divrem(c, n, ld<1>(c, in + 80), q);
        st(c, q, out);
        st(c, n, out + 80);
    } else if constexpr (OP == OP_DIVREM11) {
        Mp<1> n = ld<1>(c, in), q;
        mp_divrem(c, n, ld<1>(c, in + 40), q);
        st(c, q, out);
        st(c, n, out + 40);
    } else if constexpr (OP == OP_DIVREM22) {
        Mp<2> n = ld<2>(c, in), q;
        mp_divrem(c, n, ld<2>(c, in + 80), q);
        st(c, q, out);
        st(c, n, out + 80);
    } else if constexpr (OP == OP_WORD) {
        Mp<2> v = ld<2>(c, in);
        const uint32_t W = in[80];              // > 0 (the host refuses a zero word)
        const WordDiv d = worddiv_make(W);
        const ModW mw = modw_make(c, W);
        const uint32_t m = mp_mod_word(c, v, d), f1 = mp_mod_word_fast(c, mp_resize<1>(v), mw), f2 = mp_mod_word_fast(c, v, mw);
        const uint32_t r = mp_divrem_word(c, v, d);
        st(c, v, out);
        if (c.gl == 0) {
            out[80] = r;
            out[81] = m;
            out[82] = f1;
            out[83] = f2;
        }
    } else if constexpr (OP == OP_PRIMORIAL) {
        const uint32_t r = mp_mod_primorial(c, ld<1>(c, in));
        if (c.gl == 0) out[0] = r;
    } else if constexpr (OP == OP_DIVEXACT) {
        Mp<2> q;
        mp_divexact(c, ld<2>(c, in), ld<1>(c, in + 80), q, (int)in[120]);
        st(c, q, out);
    } else if constexpr (OP == OP_XGCD) {
        Euclid<1> e;
        e.x = ld<1>(c, in);
        e.y = ld<1>(c, in + 40);
        mp_zero(e.ux);
        mp_set_word(c, e.uy, 1);
        e.sx = -1;
        e.sy = 1;
        euclid_run(c, e, -1);
        st(c, e.x, out);
        st(c, e.ux, out + 40);
        if (c.gl == 0) out[80] = (uint32_t)e.sx;
    }
}

template <int OP>
__global__ void __launch_bounds__(64) k_group(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint8_t *__restrict__ slot_active,
                                              int n_groups, uint32_t *status) {
    __shared__ uint32_t lds[G * SCRATCH_WORDS];
    const int g = (int)blockIdx.x * (64 / G) + (int)(threadIdx.x / G);
    if (g >= n_groups || !slot_active[g]) return;
    Ctx c;
    const int lane = (int)(threadIdx.x & 63);
    c.gl = lane & (G - 1);
    c.base4 = (lane & ~(G - 1)) << 2;
    c.scr = lds + (threadIdx.x / G) * SCRATCH_WORDS;
    c.status = status;
    run_op<OP>(c, in + (size_t)g * OP_WORDS[OP][0], out + (size_t)g * OP_WORDS[OP][1]);
}

// ---------------------------------------------------------------------------- the workgroup-served remainder sequence
// workgroup b runs pairs [b WG_GROUPS, ...): group gi takes pair min(gi, count - 1) of its workgroup, so every group takes
// part in every barrier (as tests/hostsim/sim.cpp: sim_euclid_wg)
__global__ void __launch_bounds__(WG_BLOCK) k_euclid_wg(const uint32_t *__restrict__ x, const uint32_t *__restrict__ y, int count,
                                                        const int *__restrict__ stop, uint32_t *__restrict__ out, int *__restrict__ sign,
                                                        uint32_t *status) {
    __shared__ uint32_t lds[cofhe_k::WG_CTX_LDS_WORDS];
    Ctx c = cofhe_k::make_served_ctx(lds);
    c.status = status;
    const int first = (int)blockIdx.x * WG_GROUPS;
    const int mine = count - first < WG_GROUPS ? count - first : WG_GROUPS;      // >= 1: the grid covers count
    const int i = first + (c.gi < mine ? c.gi : mine - 1);
    Euclid<1> e;
    e.x = ld<1>(c, x + (size_t)40 * i);
    e.y = ld<1>(c, y + (size_t)40 * i);
    mp_zero(e.ux);
    mp_set_word(c, e.uy, 1);
    e.sx = -1;
    e.sy = 1;
    euclid_run_wg(c, e, stop[i]);
    if (c.gi < mine) {
        st(c, e.x, out + (size_t)160 * i);
        st(c, e.y, out + (size_t)160 * i + 40);
        st(c, e.ux, out + (size_t)160 * i + 80);
        st(c, e.uy, out + (size_t)160 * i + 120);
        if (c.gl == 0) {
            sign[2 * i] = e.sx;
            sign[2 * i + 1] = e.sy;
        }
    }
}

// ---------------------------------------------------------------------------- wide layout: one number per wavefront
using namespace cofhe::wide;
enum WOp { W_MUL, W_LINCOMB, W_SHIFT, W_CMP, W_MOD, W_DIVEXACT, W_EUCLID, W_COUNT };
// words per wavefront: input, output
constexpr int W_WORDS[W_COUNT][2] = {
    {256, 128},                     // MUL: x[128] y[128] -> x y
    {258, 258},                     // LINCOMB: x y A B -> A x - B y | A x + B y | word of the difference, of the sum
    {129, 257},                     // SHIFT: x n -> x << n | x >> n | bit length
    {256, 1},                       // CMP: x y -> w_cmp
    {256, 129},                     // MOD: num den -> num mod den | ok
    {257, 129},                     // DIVEXACT: num den nq -> quot | ok
    {257, 515},                     // EUCLID: x y stop -> x | y | ux | uy | sx sy | w_euclid's flag
};

__device__ WN ldw(const uint32_t *w) {
    const uint32_t l = threadIdx.x & 63u;
    return WN{w[2 * l], w[2 * l + 1]};
}
__device__ void stw(const WN &x, uint32_t *w) {
    const uint32_t l = threadIdx.x & 63u;
    w[2 * l] = x.a;
    w[2 * l + 1] = x.b;
}
__device__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }     // wave-uniform parameters

template <int OP>
__global__ void k_wide(const uint32_t *__restrict__ in_, uint32_t *__restrict__ out_, int n) {
    const int w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (w >= n) return;                                     // whole wavefronts
    const bool lane0 = (threadIdx.x & 63u) == 0;
    const uint32_t *in = in_ + (size_t)w * W_WORDS[OP][0];
    uint32_t *out = out_ + (size_t)w * W_WORDS[OP][1];
    if constexpr (OP == W_MUL) {
        stw(w_mul(ldw(in), ldw(in + 128)), out);
    } else if constexpr (OP == W_LINCOMB) {
        const uint32_t A = uni(in[256]), B = uni(in[257]);
        WN o;
        const uint32_t ws = w_lincomb_sub(o, A, ldw(in), B, ldw(in + 128));
        stw(o, out);
        const uint32_t wa = w_lincomb_add(o, A, ldw(in), B, ldw(in + 128));
        stw(o, out + 128);
        if (lane0) {
            out[256] = ws;
            out[257] = wa;
        }
    } else if constexpr (OP == W_SHIFT) {
        const WN a = ldw(in);
        const int s = (int)uni(in[128]);
        stw(w_shl(a, s), out);
        stw(w_shr(a, s), out + 128);
        const int b = w_bitlen(a);
        if (lane0) out[256] = (uint32_t)b;
    } else if constexpr (OP == W_CMP) {
        const int cm = w_cmp(ldw(in), ldw(in + 128));
        if (lane0) out[0] = (uint32_t)cm;
    } else if constexpr (OP == W_MOD) {
        bool ok = true;
        stw(w_mod(ldw(in), ldw(in + 128), ok), out);
        if (lane0) out[128] = ok ? 1u : 0u;
    } else if constexpr (OP == W_DIVEXACT) {
        bool ok = true;
        stw(w_divexact(ldw(in), ldw(in + 128), (int)uni(in[256]), ok), out);
        if (lane0) out[128] = ok ? 1u : 0u;
    } else if constexpr (OP == W_EUCLID) {
        WEuclid e;
        e.x = ldw(in);
        e.y = ldw(in + 128);
        e.ux = w_zero();
        e.uy = w_word(1u);
        e.sx = -1;
        e.sy = 1;
        const bool ok = w_euclid(e, (int)uni(in[256]));
        stw(e.x, out);
        stw(e.y, out + 128);
        stw(e.ux, out + 256);
        stw(e.uy, out + 384);
        if (lane0) {
            out[512] = (uint32_t)e.sx;
            out[513] = (uint32_t)e.sy;
            out[514] = ok ? 1u : 0u;
        }
    }
}

// ---------------------------------------------------------------------------- host side
struct DevBuf {
    void *p = nullptr;
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess; }
    ~DevBuf() { if (p) (void)hipFree(p); }
};
bool up(DevBuf &b, const void *src, size_t bytes) { return b.alloc(bytes) && (bytes == 0 || hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess); }
bool zero(DevBuf &b, size_t bytes) { return b.alloc(bytes) && hipMemset(b.p, 0, bytes ? bytes : 4) == hipSuccess; }
bool down(void *dst, const DevBuf &b, size_t bytes) { return bytes == 0 || hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }

template <int OP>
void launch_group(int n_groups, const DevBuf &in, const DevBuf &out, const DevBuf &act, const DevBuf &st) {
    hipLaunchKernelGGL(k_group<OP>, dim3((unsigned)((n_groups + 7) / 8)), dim3(64), 0, 0, (const uint32_t *)in.p, (uint32_t *)out.p,
                       (const uint8_t *)act.p, n_groups, (uint32_t *)st.p);
}
template <int OP>
void launch_wide(int n, int waves, const DevBuf &in, const DevBuf &out) {
    hipLaunchKernelGGL(k_wide<OP>, dim3((unsigned)((n + waves - 1) / waves)), dim3(64u * (unsigned)waves), 0, 0, (const uint32_t *)in.p,
                       (uint32_t *)out.p, n);
}
}  // namespace

extern "C" {
int prims_gpu_wg_groups(void) { return WG_GROUPS; }
// words per group of op: io[0] in, io[1] out; -1 for an unknown op
int prims_gpu_words(int op, int *io) {
    if (op < 0 || op >= OP_COUNT) return -1;
    io[0] = OP_WORDS[op][0];
    io[1] = OP_WORDS[op][1];
    return 0;
}
int prims_gpu_wide_words(int op, int *io) {
    if (op < 0 || op >= W_COUNT) return -1;
    io[0] = W_WORDS[op][0];
    io[1] = W_WORDS[op][1];
    return 0;
}
// One launch of op over n_groups groups (eight per wavefront, 64 threads per workgroup); the groups with slot_active[g] == 0
// return at once and their output stays zero.  *status = the device status word after the launch (lane.hpp: CF_ST_*).
// Returns 0, -1 when no GPU run was possible, -2 for arguments the kernels must not see.
int prims_gpu_run(int op, const uint32_t *in, uint32_t *out, const uint8_t *slot_active, int n_groups, uint32_t *status) {
    if (op < 0 || op >= OP_COUNT || n_groups <= 0) return -2;
    const size_t wi = OP_WORDS[op][0], wo = OP_WORDS[op][1];
    if (op == OP_WORD)
        for (int g = 0; g < n_groups; g++)
            if (slot_active[g] && in[wi * g + 80] == 0) return -2;            // worddiv_make divides by the word
    DevBuf di, dout, da, ds;
    if (!(up(di, in, wi * n_groups * 4) && zero(dout, wo * n_groups * 4) && up(da, slot_active, (size_t)n_groups) && zero(ds, 4))) return -1;
    switch (op) {
        case OP_LANE: launch_group<OP_LANE>(n_groups, di, dout, da, ds); break;
        case OP_MUL11: launch_group<OP_MUL11>(n_groups, di, dout, da, ds); break;
        case OP_MUL21: launch_group<OP_MUL21>(n_groups, di, dout, da, ds); break;
        case OP_LINCOMB: launch_group<OP_LINCOMB>(n_groups, di, dout, da, ds); break;
        case OP_SHIFT: launch_group<OP_SHIFT>(n_groups, di, dout, da, ds); break;
        case OP_BITS: launch_group<OP_BITS>(n_groups, di, dout, da, ds); break;
        case OP_DIVREM21: launch_group<OP_DIVREM21>(n_groups, di, dout, da, ds); break;
        case OP_DIVREM11: launch_group<OP_DIVREM11>(n_groups, di, dout, da, ds); break;
        case OP_DIVREM22: launch_group<OP_DIVREM22>(n_groups, di, dout, da, ds); break;
        case OP_WORD: launch_group<OP_WORD>(n_groups, di, dout, da, ds); break;
        case OP_PRIMORIAL: launch_group<OP_PRIMORIAL>(n_groups, di, dout, da, ds); break;
        case OP_DIVEXACT: launch_group<OP_DIVEXACT>(n_groups, di, dout, da, ds); break;
        default: launch_group<OP_XGCD>(n_groups, di, dout, da, ds); break;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    return down(out, dout, wo * n_groups * 4) && down(status, ds, 4) ? 0 : -1;
}
// euclid_run_wg on `count` pairs (x[40], y[40]), WG_GROUPS pairs per workgroup of WG_BLOCK threads; stop < 0: down to the
// gcd.  out per pair: x[40] y[40] ux[40] uy[40]; sign[2 i], sign[2 i + 1] = sx, sy (as sim_euclid_wg)
int prims_gpu_euclid_wg(const uint32_t *x, const uint32_t *y, int count, const int *stop, uint32_t *out, int *sign, uint32_t *status) {
    if (count <= 0) return -2;
    DevBuf dx, dy, dst, dout, dsg, ds;
    if (!(up(dx, x, (size_t)count * 160) && up(dy, y, (size_t)count * 160) && up(dst, stop, (size_t)count * 4) && zero(dout, (size_t)count * 640) &&
          zero(dsg, (size_t)count * 8) && zero(ds, 4)))
        return -1;
    hipLaunchKernelGGL(k_euclid_wg, dim3((unsigned)((count + WG_GROUPS - 1) / WG_GROUPS)), dim3(WG_BLOCK), 0, 0, (const uint32_t *)dx.p,
                       (const uint32_t *)dy.p, count, (const int *)dst.p, (uint32_t *)dout.p, (int *)dsg.p, (uint32_t *)ds.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    return down(out, dout, (size_t)count * 640) && down(sign, dsg, (size_t)count * 8) && down(status, ds, 4) ? 0 : -1;
}
// One launch of a wide op over n numbers, one per wavefront, waves_per_block (1 or 4) wavefronts per workgroup
int prims_gpu_wide(int op, const uint32_t *in, uint32_t *out, int n, int waves_per_block) {
    if (op < 0 || op >= W_COUNT || n <= 0 || waves_per_block < 1 || waves_per_block > 16) return -2;
    const size_t wi = W_WORDS[op][0], wo = W_WORDS[op][1];
    DevBuf di, dout;
    if (!(up(di, in, wi * n * 4) && zero(dout, wo * n * 4))) return -1;
    switch (op) {
        case W_MUL: launch_wide<W_MUL>(n, waves_per_block, di, dout); break;
        case W_LINCOMB: launch_wide<W_LINCOMB>(n, waves_per_block, di, dout); break;
        case W_SHIFT: launch_wide<W_SHIFT>(n, waves_per_block, di, dout); break;
        case W_CMP: launch_wide<W_CMP>(n, waves_per_block, di, dout); break;
        case W_MOD: launch_wide<W_MOD>(n, waves_per_block, di, dout); break;
        case W_DIVEXACT: launch_wide<W_DIVEXACT>(n, waves_per_block, di, dout); break;
        default: launch_wide<W_EUCLID>(n, waves_per_block, di, dout); break;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    return down(out, dout, wo * n * 4) ? 0 : -1;
}
}
