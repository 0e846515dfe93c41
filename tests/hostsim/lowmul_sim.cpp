// Host build of the low-half products (cofhe_amd/csrc/mp.hpp: mp_mul_low2) and of nucomp_m12 on both of its routes
// (cofhe_amd/csrc/qf.hpp) with COFHE_HOSTSIM: the 8 lanes of a limb group as 8 host threads, as tests/hostsim/sim.cpp runs
// them.  Record layouts are those of tests/gpu_kernels/lowmul_gpu.hip (tests/lowmul_cases.py packs for both tiers).
// TEST INFRASTRUCTURE ONLY; not linked into the product library.
#define COFHE_HOSTSIM 1
#include <cstring>
#include <thread>
#include <vector>

#include "../../cofhe_amd/csrc/qf.hpp"

using namespace cofhe;

template <typename F>
static void run_group(F &&fn) {
    static GroupShared gs;
    std::vector<std::thread> th;
    for (int l = 0; l < G; l++)
        th.emplace_back([&, l]() {
            Ctx c;
            c.gl = l;
            c.gs = &gs;
            c.sense = gs.bar.sense.load();
            fn(c);
        });
    for (auto &t : th) t.join();
}

template <int P>
static Mp<P> ld(const Ctx &c, const uint32_t *w) {
    Mp<P> x;
    for (int p = 0; p < P; p++)
        for (int j = 0; j < CH; j++) x.v[p][j] = w[p * PLIMBS + c.gl * CH + j];
    return x;
}
template <int P>
static void st(const Ctx &c, const Mp<P> &x, uint32_t *w) {
    for (int p = 0; p < P; p++)
        for (int j = 0; j < CH; j++) w[p * PLIMBS + c.gl * CH + j] = x.v[p][j];
}

constexpr int MUL_IN = 160, MUL_OUT = 40, M12_IN = 322, M12_OUT = 123;

extern "C" {
unsigned lowmul_sim_status(void) { return g_sim_status.exchange(0); }
int lowmul_sim_compiled_in(void) { return M12_LOW_HALF ? 1 : 0; }
// the bound and the predicate by themselves (qf.hpp: m12_bound, m12_low_half_serves)
int lowmul_sim_bound(int bx0, int by0, int bx1, int by1, int bv1) { return m12_bound(bx0, by0, bx1, by1, bv1); }
int lowmul_sim_serves(int nb, uint32_t v1_limb0) { return m12_low_half_serves(nb, v1_limb0) ? 1 : 0; }

// in: x0[40] y0[40] x1[40] y1[40] -> out[40]: x0 y0 mod 2^640 in limbs 0..19, x1 y1 mod 2^640 in limbs 20..39
void lowmul_sim_mul(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) {
            const uint32_t *r = in + (size_t)MUL_IN * i;
            st(c, mp_mul_low2(c, ld<1>(c, r), ld<1>(c, r + 40), ld<1>(c, r + 80), ld<1>(c, r + 120)), out + (size_t)MUL_OUT * i);
        }
    });
}
// in: R[40] |C|[40] v1[40] v2[40] |m|[40] |s|[40] c2d[80] signs (bit 0: C, 1: m, 2: s) try_low
// out: |M1|[40] |M2|[80] sign of M1, of M2, 1 when the low-half route was taken
void lowmul_sim_m12(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) {
            const uint32_t *r = in + (size_t)M12_IN * i;
            uint32_t *o = out + (size_t)M12_OUT * i;
            const uint32_t sg = r[320];
            const Mp<1> R = ld<1>(c, r), v1 = ld<1>(c, r + 80), v2 = ld<1>(c, r + 120);
            const SMp<1> C{ld<1>(c, r + 40), (int)(sg & 1u)}, m{ld<1>(c, r + 160), (int)((sg >> 1) & 1u)}, s{ld<1>(c, r + 200), (int)((sg >> 2) & 1u)};
            const Mp<2> c2d = ld<2>(c, r + 240);
            SMp<1> M1;
            SMp<2> M2;
            const bool low = nucomp_m12(c, M1, M2, R, C, v1, v2, m, s, c2d, mp_bitlen(c, v1), mp_bitlen(c, v2), r[321] != 0);
            st(c, M1.m, o);
            st(c, M2.m, o + 40);
            if (c.gl == 0) {
                o[120] = (uint32_t)M1.neg;
                o[121] = (uint32_t)M2.neg;
                o[122] = low ? 1u : 0u;
            }
        }
    });
}
}
