// Host build of the paired 2-adic division (cofhe_amd/csrc/mp.hpp: mp_divexact_pair; qf.hpp: m12_low_quot_pair), of
// mp_divexact with a one-plane numerator, of mp_sqr_low and of nucomp_m12, nucomp_ab and nucomp_c with COFHE_HOSTSIM: the 8
// lanes of a limb group as 8 host threads, as tests/hostsim/sim.cpp runs them.  Record layouts are those of
// tests/gpu_kernels/pairdiv_gpu.hip (tests/pairdiv_cases.py, lowmul_cases.py and onep_cases.py pack for both tiers).
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

enum Op { OP_DIVP, OP_QUOTP, OP_DIVX, OP_SQR, OP_M12, OP_AB, OP_C, OP_COUNT };
constexpr int OP_WORDS[OP_COUNT][2] = {{81, 40}, {124, 42}, {81, 40}, {40, 40}, {322, 123}, {322, 163}, {161, 81}};

static void run_op(Ctx &c, int op, const uint32_t *in, uint32_t *out) {
    switch (op) {
    case OP_DIVP:       // num (pair)[40] den[40] nq -> quotients (pair)[40]
        st(c, mp_divexact_pair(c, ld<1>(c, in), ld<1>(c, in + 40), (int)in[80]), out);
        break;
    case OP_QUOTP: {    // pa[40] pb[40] v1[40] sub0 sub1 nb0 nb1 -> |M1| | |M2| (pair)[40] neg0 neg1
        const M12Pair r = m12_low_quot_pair(c, ld<1>(c, in), ld<1>(c, in + 40), in[120] != 0, in[121] != 0, ld<1>(c, in + 80), (int)in[122], (int)in[123]);
        st(c, r.m, out);
        if (c.gl == 0) {
            out[40] = (uint32_t)r.neg0;
            out[41] = (uint32_t)r.neg1;
        }
        break;
    }
    case OP_DIVX: {     // num[40] den[40] nq -> quot[40]
        Mp<1> q;
        mp_divexact(c, ld<1>(c, in), ld<1>(c, in + 40), q, (int)in[80]);
        st(c, q, out);
        break;
    }
    case OP_SQR:        // x[40] -> x^2 mod 2^1280
        st(c, mp_sqr_low(c, ld<1>(c, in)), out);
        break;
    case OP_M12: {      // as tests/hostsim/lowmul_sim.cpp
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
        break;
    }
    case OP_AB: {       // as tests/hostsim/onep_sim.cpp
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
        break;
    }
    default: {          // OP_C, as tests/hostsim/onep_sim.cpp
        const QDisc dd{in + 80, (int)in[160]};
        Mp<2> cn;
        const bool low = nucomp_c(c, cn, ld<1>(c, in), ld<1>(c, in + 40), dd);
        st(c, cn, out);
        if (c.gl == 0) out[80] = low ? 1u : 0u;
        break;
    }
    }
}

extern "C" {
unsigned pairdiv_sim_status(void) { return g_sim_status.exchange(0); }
// bit 0: the paired division, 1: no high-limb bookkeeping for a one-plane numerator, 2: the square from every pair once
int pairdiv_sim_compiled_in(void) { return (M12_LOW_HALF && M12_PAIRED_DIV ? 1 : 0) | (DIVEXACT_HIGH_ALWAYS ? 0 : 2) | (SQR_EACH_PAIR_ONCE ? 4 : 0); }
int pairdiv_sim_words(int op, int *io) {
    if (op < 0 || op >= OP_COUNT) return -1;
    io[0] = OP_WORDS[op][0];
    io[1] = OP_WORDS[op][1];
    return 0;
}
// count records of op, one after the other in one group
int pairdiv_sim_run(int op, const uint32_t *in, uint32_t *out, int count) {
    if (op < 0 || op >= OP_COUNT) return -2;
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) run_op(c, op, in + (size_t)OP_WORDS[op][0] * i, out + (size_t)OP_WORDS[op][1] * i);
    });
    return 0;
}
}
