// onep_gpu.hip -- TEST INFRASTRUCTURE: the one-plane tail of the composition -- mp_mul_half2 and mp_sqr_low
// (cofhe_amd/csrc/mp.hpp), nucomp_ab and nucomp_c on both of their routes (cofhe_amd/csrc/qf.hpp) -- run ON THE GPU against
// Python integers (tests/test_gpu_onep.py).  What the host simulator (tests/hostsim/onep_sim.cpp) replaces is exactly what
// can only go wrong here: the stores of half a group into the LDS slice, the windows that come back four lanes away, and the
// route decisions under any_lane -- on the device a ballot over the WHOLE wavefront, so one group outside a bound sends its
// seven neighbours through the double-width route.
//
// Layout as tests/gpu_kernels/lowmul_gpu.hip: 64 threads per workgroup, one instance per 8-lane group, a map
// slot_active[n_groups] whose switched-off groups return at once.  Record layouts as tests/hostsim/onep_sim.cpp.
// Built by __graft_entry__.build() into tests/gpu_kernels/libonep_gpu.so.  Not part of the product.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../cofhe_amd/csrc/qf.hpp"

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

enum Op { OP_MUL, OP_SQR, OP_AB, OP_C, OP_COUNT };
constexpr int OP_WORDS[OP_COUNT][2] = {
    {160, 80},                      // MUL: x0[40] y0[40] x1[40] y1[40] -> x0 y0 [40] | x1 y1 [40] (of the low 640 bits of each operand)
    {40, 40},                       // SQR: x[40] -> x^2 mod 2^1280
    {322, 163},                     // AB: R1 |C1| R0 |C0| |M1| [40 each] |M2|[80] |b1|[40] signs m2_one_plane -> |a'|[80] |b'|[80] sign, sign, one-plane route taken
    {161, 81},                      // C: a'[40] |b'|[40] |Delta|[80] half_dbits -> c'[80], low half taken
};

template <int OP>
__device__ void run_op(Ctx &c, const uint32_t *in, uint32_t *out) {
    if constexpr (OP == OP_MUL) {
        const MpPair pp = mp_mul_half2(c, ld<1>(c, in), ld<1>(c, in + 40), ld<1>(c, in + 80), ld<1>(c, in + 120));
        st(c, pp.p0, out);
        st(c, pp.p1, out + 40);
    } else if constexpr (OP == OP_SQR) {
        st(c, mp_sqr_low(c, ld<1>(c, in)), out);
    } else if constexpr (OP == OP_AB) {
        const uint32_t sg = in[320];
        const Mp<1> R1 = ld<1>(c, in), R0 = ld<1>(c, in + 80);
        const SMp<1> C1{ld<1>(c, in + 40), (int)(sg & 1u)}, C0{ld<1>(c, in + 120), (int)((sg >> 1) & 1u)},
            M1{ld<1>(c, in + 160), (int)((sg >> 2) & 1u)}, b1{ld<1>(c, in + 280), (int)((sg >> 4) & 1u)};
        const SMp<2> M2{ld<2>(c, in + 200), (int)((sg >> 3) & 1u)};
        SMp<2> an, bn;
        const bool one = nucomp_ab(c, an, bn, R1, C1, R0, C0, M1, M2, b1, in[321] != 0);
        st(c, an.m, out);
        st(c, bn.m, out + 80);
        if (c.gl == 0) {
            out[160] = (uint32_t)an.neg;
            out[161] = (uint32_t)bn.neg;
            out[162] = one ? 1u : 0u;
        }
    } else {
        const QDisc dd{in + 80, (int)in[160]};
        Mp<2> cn;
        const bool low = nucomp_c(c, cn, ld<1>(c, in), ld<1>(c, in + 40), dd);
        st(c, cn, out);
        if (c.gl == 0) out[80] = low ? 1u : 0u;
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
}  // namespace

extern "C" {
int onep_gpu_compiled_in(void) { return (DOT_ONE_PLANE ? 1 : 0) | (C_LOW_HALF ? 2 : 0); }
// words per group of op: io[0] in, io[1] out; -1 for an unknown op
int onep_gpu_words(int op, int *io) {
    if (op < 0 || op >= OP_COUNT) return -1;
    io[0] = OP_WORDS[op][0];
    io[1] = OP_WORDS[op][1];
    return 0;
}
// One launch of op over n_groups groups (eight per wavefront); the groups with slot_active[g] == 0 return at once and their
// output stays zero.  *status = the device status word after the launch.  Returns 0, -1 when no GPU run was possible, -2
// for arguments the kernels must not see.
int onep_gpu_run(int op, const uint32_t *in, uint32_t *out, const uint8_t *slot_active, int n_groups, uint32_t *status) {
    if (op < 0 || op >= OP_COUNT || n_groups <= 0) return -2;
    const size_t wi = OP_WORDS[op][0], wo = OP_WORDS[op][1];
    DevBuf di, dout, da, ds;
    if (!(up(di, in, wi * n_groups * 4) && zero(dout, wo * n_groups * 4) && up(da, slot_active, (size_t)n_groups) && zero(ds, 4))) return -1;
    if (op == OP_MUL) launch_group<OP_MUL>(n_groups, di, dout, da, ds);
    else if (op == OP_SQR) launch_group<OP_SQR>(n_groups, di, dout, da, ds);
    else if (op == OP_AB) launch_group<OP_AB>(n_groups, di, dout, da, ds);
    else launch_group<OP_C>(n_groups, di, dout, da, ds);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    return down(out, dout, wo * n_groups * 4) && down(status, ds, 4) ? 0 : -1;
}
}
