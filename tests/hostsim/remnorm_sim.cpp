// Host build of the remainder-only long division (cofhe_amd/csrc/mp.hpp: mp_rem_norm), of mp_divrem_norm beside it and of the
// step r = y1 m mod a1 of the composition (qf.hpp: smp_mul, smod with its remainder-only flag) with COFHE_HOSTSIM: the 8 lanes
// of a limb group as 8 host threads, as tests/hostsim/sim.cpp runs them.  Record layouts are those of
// tests/gpu_kernels/remnorm_gpu.hip (tests/remnorm_cases.py packs for both tiers).
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

enum Op { OP_REM2, OP_DIVREM2, OP_REM1, OP_STEP, OP_COUNT };
constexpr int OP_WORDS[OP_COUNT][2] = {{120, 80}, {120, 80}, {80, 40}, {121, 40}};

static void run_op(Ctx &c, int op, const uint32_t *in, uint32_t *out) {
    switch (op) {
    case OP_REM2: {     // num[80] den[40] -> num mod den [80], by mp_rem_norm
        Mp<2> n = ld<2>(c, in);
        const Mp<1> d = ld<1>(c, in + 80);
        mp_rem_norm(c, n, d, mp_bitlen(c, d));
        st(c, n, out);
        break;
    }
    case OP_DIVREM2: {  // the same by mp_divrem_norm (its quotient dropped)
        Mp<2> n = ld<2>(c, in), q;
        const Mp<1> d = ld<1>(c, in + 80);
        mp_divrem_norm(c, n, d, mp_bitlen(c, d), q);
        st(c, n, out);
        break;
    }
    case OP_REM1: {     // num[40] den[40] -> num mod den [40]
        Mp<1> n = ld<1>(c, in);
        const Mp<1> d = ld<1>(c, in + 40);
        mp_rem_norm(c, n, d, mp_bitlen(c, d));
        st(c, n, out);
        break;
    }
    default: {          // OP_STEP: |y1|[40] |m|[40] a1[40] signs (bit 0: y1, bit 1: m) -> y1 m mod a1 [40], as qf_compose computes it
        const SMp<1> y1{ld<1>(c, in), (int)(in[120] & 1u)}, m{ld<1>(c, in + 40), (int)((in[120] >> 1) & 1u)};
        const SMp<2> t = smp_mul(c, y1, m);
        st(c, smod<true>(c, t, ld<1>(c, in + 80)), out);
        break;
    }
    }
}

extern "C" {
unsigned remnorm_sim_status(void) { return g_sim_status.exchange(0); }
int remnorm_sim_compiled_in(void) { return REM_NORM ? 1 : 0; }
int remnorm_sim_words(int op, int *io) {
    if (op < 0 || op >= OP_COUNT) return -1;
    io[0] = OP_WORDS[op][0];
    io[1] = OP_WORDS[op][1];
    return 0;
}
// digits, add-backs and steps through the general carry resolve of mp_rem_norm since the last call
void remnorm_sim_stats(long *out) {
    out[0] = g_stats.rem_steps;
    out[1] = g_stats.rem_addbacks;
    out[2] = g_stats.rem_fallbacks;
    memset(&g_stats, 0, sizeof(g_stats));
}
// count records of op, one after the other in one group
int remnorm_sim_run(int op, const uint32_t *in, uint32_t *out, int count) {
    if (op < 0 || op >= OP_COUNT) return -2;
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) run_op(c, op, in + (size_t)OP_WORDS[op][0] * i, out + (size_t)OP_WORDS[op][1] * i);
    });
    return 0;
}
}
