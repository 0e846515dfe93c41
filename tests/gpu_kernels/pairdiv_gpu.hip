// pairdiv_gpu.hip -- TEST INFRASTRUCTURE: the paired 2-adic division (cofhe_amd/csrc/mp.hpp: mp_divexact_pair; qf.hpp:
// m12_low_quot_pair), mp_divexact with a one-plane numerator, mp_sqr_low and nucomp_m12, nucomp_ab, nucomp_c run ON THE GPU
// against Python integers (tests/test_gpu_pairdiv.py).  What the host simulator (tests/hostsim/pairdiv_sim.cpp) replaces is
// exactly what can only go wrong here: the row_shr:4 copy of the divisor into the upper half, the quad broadcast of a half's
// two lowest limbs, the row moves patched at the edges of a half, the ballots cut between lane 3 and lane 4, and the route
// decision under any_lane.
//
// Layout as tests/gpu_kernels/lowmul_gpu.hip: 64 threads per workgroup, one instance per 8-lane group, a map
// slot_active[n_groups] whose switched-off groups return at once.  Record layouts as tests/hostsim/pairdiv_sim.cpp.
// Built by __graft_entry__.build() into tests/gpu_kernels/libpairdiv_gpu.so.  Not part of the product.
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

enum Op { OP_DIVP, OP_QUOTP, OP_DIVX, OP_SQR, OP_M12, OP_AB, OP_C, OP_COUNT };
constexpr int OP_WORDS[OP_COUNT][2] = {{81, 40}, {124, 42}, {81, 40}, {40, 40}, {322, 123}, {322, 163}, {161, 81}};

template <int OP>
__device__ void run_op(Ctx &c, const uint32_t *in, uint32_t *out) {
    if constexpr (OP == OP_DIVP) {
        st(c, mp_divexact_pair(c, ld<1>(c, in), ld<1>(c, in + 40), (int)in[80]), out);
    } else if constexpr (OP == OP_QUOTP) {
        const M12Pair r = m12_low_quot_pair(c, ld<1>(c, in), ld<1>(c, in + 40), in[120] != 0, in[121] != 0, ld<1>(c, in + 80), (int)in[122], (int)in[123]);
        st(c, r.m, out);
        if (c.gl == 0) {
            out[40] = (uint32_t)r.neg0;
            out[41] = (uint32_t)r.neg1;
        }
    } else if constexpr (OP == OP_DIVX) {
        Mp<1> q;
        mp_divexact(c, ld<1>(c, in), ld<1>(c, in + 40), q, (int)in[80]);
        st(c, q, out);
    } else if constexpr (OP == OP_SQR) {
        st(c, mp_sqr_low(c, ld<1>(c, in)), out);
    } else if constexpr (OP == OP_M12) {
        const uint32_t sg = in[320];
        const Mp<1> R = ld<1>(c, in), v1 = ld<1>(c, in + 80), v2 = ld<1>(c, in + 120);
        const SMp<1> C{ld<1>(c, in + 40), (int)(sg & 1u)}, m{ld<1>(c, in + 160), (int)((sg >> 1) & 1u)}, s{ld<1>(c, in + 200), (int)((sg >> 2) & 1u)};
        const Mp<2> c2d = ld<2>(c, in + 240);
        SMp<1> M1;
        SMp<2> M2;
        const bool low = nucomp_m12(c, M1, M2, R, C, v1, v2, m, s, c2d, mp_bitlen(c, v1), mp_bitlen(c, v2), in[321] != 0);
        st(c, M1.m, out);
        st(c, M2.m, out + 40);
        if (c.gl == 0) {
            out[120] = (uint32_t)M1.neg;
            out[121] = (uint32_t)M2.neg;
            out[122] = low ? 1u : 0u;
        }
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
// bit 0: the paired division, 1: no high-limb bookkeeping for a one-plane numerator, 2: the square from every pair once
int pairdiv_gpu_compiled_in(void) { return (M12_LOW_HALF && M12_PAIRED_DIV ? 1 : 0) | (DIVEXACT_HIGH_ALWAYS ? 0 : 2) | (SQR_EACH_PAIR_ONCE ? 4 : 0); }
// words per group of op: io[0] in, io[1] out; -1 for an unknown op
int pairdiv_gpu_words(int op, int *io) {
    if (op < 0 || op >= OP_COUNT) return -1;
    io[0] = OP_WORDS[op][0];
    io[1] = OP_WORDS[op][1];
    return 0;
}
// One launch of op over n_groups groups (eight per wavefront); the groups with slot_active[g] == 0 return at once and their
// output stays zero.  *status = the device status word after the launch.  Returns 0, -1 when no GPU run was possible, -2
// for arguments the kernels must not see.
int pairdiv_gpu_run(int op, const uint32_t *in, uint32_t *out, const uint8_t *slot_active, int n_groups, uint32_t *status) {
    if (op < 0 || op >= OP_COUNT || n_groups <= 0) return -2;
    const size_t wi = OP_WORDS[op][0], wo = OP_WORDS[op][1];
    DevBuf di, dout, da, ds;
    if (!(up(di, in, wi * n_groups * 4) && zero(dout, wo * n_groups * 4) && up(da, slot_active, (size_t)n_groups) && zero(ds, 4))) return -1;
    switch (op) {
    case OP_DIVP: launch_group<OP_DIVP>(n_groups, di, dout, da, ds); break;
    case OP_QUOTP: launch_group<OP_QUOTP>(n_groups, di, dout, da, ds); break;
    case OP_DIVX: launch_group<OP_DIVX>(n_groups, di, dout, da, ds); break;
    case OP_SQR: launch_group<OP_SQR>(n_groups, di, dout, da, ds); break;
    case OP_M12: launch_group<OP_M12>(n_groups, di, dout, da, ds); break;
    case OP_AB: launch_group<OP_AB>(n_groups, di, dout, da, ds); break;
    default: launch_group<OP_C>(n_groups, di, dout, da, ds); break;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    return down(out, dout, wo * n_groups * 4) && down(status, ds, 4) ? 0 : -1;
}
}
