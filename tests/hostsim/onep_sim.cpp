// Host build of the one-plane tail of the composition -- mp_mul_half2 and mp_sqr_low (cofhe_amd/csrc/mp.hpp), nucomp_ab and
// nucomp_c on both of their routes (cofhe_amd/csrc/qf.hpp) -- with COFHE_HOSTSIM: the 8 lanes of a limb group as 8 host
// threads, as tests/hostsim/sim.cpp runs them.  Record layouts are those of tests/gpu_kernels/onep_gpu.hip
// (tests/onep_cases.py packs for both tiers).  TEST INFRASTRUCTURE ONLY; not linked into the product library.
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

constexpr int MUL_IN = 160, MUL_OUT = 80, SQR_IN = 40, SQR_OUT = 40, AB_IN = 322, AB_OUT = 163, C_IN = 161, C_OUT = 81;

extern "C" {
unsigned onep_sim_status(void) { return g_sim_status.exchange(0); }
int onep_sim_compiled_in(void) { return (DOT_ONE_PLANE ? 1 : 0) | (C_LOW_HALF ? 2 : 0); }
// the predicates by themselves (qf.hpp: dot_one_plane_serves, c_low_bound, c_low_serves)
int onep_sim_dot_serves(int bR, int bC, int bM1, int bM2) { return dot_one_plane_serves(bR, bC, bM1, bM2) ? 1 : 0; }
int onep_sim_c_bound(int bb, int dbits, int ba) { return c_low_bound(bb, dbits, ba); }
int onep_sim_c_serves(int nbc, uint32_t a_limb0) { return c_low_serves(nbc, a_limb0) ? 1 : 0; }

// in: x0[40] y0[40] x1[40] y1[40] -> out: x0 y0 [40] x1 y1 [40] for the low 640 bits of every operand
void onep_sim_mul(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) {
            const uint32_t *r = in + (size_t)MUL_IN * i;
            const MpPair pp = mp_mul_half2(c, ld<1>(c, r), ld<1>(c, r + 40), ld<1>(c, r + 80), ld<1>(c, r + 120));
            st(c, pp.p0, out + (size_t)MUL_OUT * i);
            st(c, pp.p1, out + (size_t)MUL_OUT * i + 40);
        }
    });
}
// in: x[40] -> out: x^2 mod 2^1280
void onep_sim_sqr(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) st(c, mp_sqr_low(c, ld<1>(c, in + (size_t)SQR_IN * i)), out + (size_t)SQR_OUT * i);
    });
}
// in: R1[40] |C1|[40] R0[40] |C0|[40] |M1|[40] |M2|[80] |b1|[40] signs (bit 0: C1, 1: C0, 2: M1, 3: M2, 4: b1) m2_one_plane
// out: |a'|[80] |b'|[80] sign of a', of b', 1 when the one-plane route was taken
void onep_sim_ab(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) {
            const uint32_t *r = in + (size_t)AB_IN * i;
            uint32_t *o = out + (size_t)AB_OUT * i;
            const uint32_t sg = r[320];
            const Mp<1> R1 = ld<1>(c, r), R0 = ld<1>(c, r + 80);
            const SMp<1> C1{ld<1>(c, r + 40), (int)(sg & 1u)}, C0{ld<1>(c, r + 120), (int)((sg >> 1) & 1u)},
                M1{ld<1>(c, r + 160), (int)((sg >> 2) & 1u)}, b1{ld<1>(c, r + 280), (int)((sg >> 4) & 1u)};
            const SMp<2> M2{ld<2>(c, r + 200), (int)((sg >> 3) & 1u)};
            SMp<2> an, bn;
            const bool one = nucomp_ab(c, an, bn, R1, C1, R0, C0, M1, M2, b1, r[321] != 0);
            st(c, an.m, o);
            st(c, bn.m, o + 80);
            if (c.gl == 0) {
                o[160] = (uint32_t)an.neg;
                o[161] = (uint32_t)bn.neg;
                o[162] = one ? 1u : 0u;
            }
        }
    });
}
// in: a'[40] |b'|[40] |Delta|[80] half_dbits -> out: c'[80], 1 when it came from the low half
void onep_sim_c(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) {
            const uint32_t *r = in + (size_t)C_IN * i;
            uint32_t *o = out + (size_t)C_OUT * i;
            const QDisc dd{r + 80, (int)r[160]};
            Mp<2> cn;
            const bool low = nucomp_c(c, cn, ld<1>(c, r), ld<1>(c, r + 40), dd);
            st(c, cn, o);
            if (c.gl == 0) o[80] = low ? 1u : 0u;
        }
    });
}
}
