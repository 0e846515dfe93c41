// remnorm_gpu.hip -- TEST INFRASTRUCTURE: the remainder-only long division (cofhe_amd/csrc/mp.hpp: mp_rem_norm with
// mp_lincomb_sub_carry_sparse), mp_divrem_norm beside it and the step r = y1 m mod a1 of the composition (qf.hpp: smp_mul, smod
// with its remainder-only flag) run ON THE GPU against Python integers (tests/test_gpu_remnorm.py).  What the host simulator
// (tests/hostsim/remnorm_sim.cpp) replaces is exactly what can only go wrong here: the numerator staged shifted in the LDS
// slice by lanes that store to computed addresses, the row moves that carry a limb from lane to lane, the one load per digit
// that every lane of the group issues, and the carry resolve chosen under any_lane by a wavefront whose groups divide different
// numbers with different digit counts.
//
// Layout as tests/gpu_kernels/pairdiv_gpu.hip: 64 threads per workgroup, one instance per 8-lane group, a map
// slot_active[n_groups] whose switched-off groups return at once.  Record layouts as tests/hostsim/remnorm_sim.cpp.
// Built by __graft_entry__.build() into tests/gpu_kernels/libremnorm_gpu.so.  Not part of the product.
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

enum Op { OP_REM2, OP_DIVREM2, OP_REM1, OP_STEP, OP_COUNT };
constexpr int OP_WORDS[OP_COUNT][2] = {{120, 80}, {120, 80}, {80, 40}, {121, 40}};

template <int OP>
__device__ void run_op(Ctx &c, const uint32_t *in, uint32_t *out) {
    if constexpr (OP == OP_REM2) {
        Mp<2> n = ld<2>(c, in);
        const Mp<1> d = ld<1>(c, in + 80);
        mp_rem_norm(c, n, d, mp_bitlen(c, d));
        st(c, n, out);
    } else if constexpr (OP == OP_DIVREM2) {
        Mp<2> n = ld<2>(c, in), q;
        const Mp<1> d = ld<1>(c, in + 80);
        mp_divrem_norm(c, n, d, mp_bitlen(c, d), q);
        st(c, n, out);
    } else if constexpr (OP == OP_REM1) {
        Mp<1> n = ld<1>(c, in);
        const Mp<1> d = ld<1>(c, in + 40);
        mp_rem_norm(c, n, d, mp_bitlen(c, d));
        st(c, n, out);
    } else {
        const SMp<1> y1{ld<1>(c, in), (int)(in[120] & 1u)}, m{ld<1>(c, in + 40), (int)((in[120] >> 1) & 1u)};
        const SMp<2> t = smp_mul(c, y1, m);
        st(c, smod<true>(c, t, ld<1>(c, in + 80)), out);
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
// 1: smod's remainder-only flag reaches mp_rem_norm (no -DCOFHE_REM_QUOT)
int remnorm_gpu_compiled_in(void) { return REM_NORM ? 1 : 0; }
// words per group of op: io[0] in, io[1] out; -1 for an unknown op
int remnorm_gpu_words(int op, int *io) {
    if (op < 0 || op >= OP_COUNT) return -1;
    io[0] = OP_WORDS[op][0];
    io[1] = OP_WORDS[op][1];
    return 0;
}
// One launch of op over n_groups groups (eight per wavefront); the groups with slot_active[g] == 0 return at once and their
// output stays zero.  *status = the device status word after the launch.  Returns 0, -1 when no GPU run was possible, -2
// for arguments the kernels must not see.
int remnorm_gpu_run(int op, const uint32_t *in, uint32_t *out, const uint8_t *slot_active, int n_groups, uint32_t *status) {
    if (op < 0 || op >= OP_COUNT || n_groups <= 0) return -2;
    const size_t wi = OP_WORDS[op][0], wo = OP_WORDS[op][1];
    DevBuf di, dout, da, ds;
    if (!(up(di, in, wi * n_groups * 4) && zero(dout, wo * n_groups * 4) && up(da, slot_active, (size_t)n_groups) && zero(ds, 4))) return -1;
    switch (op) {
    case OP_REM2: launch_group<OP_REM2>(n_groups, di, dout, da, ds); break;
    case OP_DIVREM2: launch_group<OP_DIVREM2>(n_groups, di, dout, da, ds); break;
    case OP_REM1: launch_group<OP_REM1>(n_groups, di, dout, da, ds); break;
    default: launch_group<OP_STEP>(n_groups, di, dout, da, ds); break;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    return down(out, dout, wo * n_groups * 4) && down(status, ds, 4) ? 0 : -1;
}
}
