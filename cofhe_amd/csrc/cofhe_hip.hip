// cofhe_hip.hip -- the gfx950 throughput kernels (launched by abi.hip, declared in kernels.hpp).
//
// Kernel geometry: 256-thread workgroups = 4 wavefronts = 32 limb groups; group g of the grid
// handles work item g (one form composition, one exponentiation, or one output coefficient of
// the plaintext-matrix x ciphertext-matrix product).  Each group owns a 208-word LDS slice
// for multiplication staging and limb shifts (26 KiB per workgroup).
#include <hip/hip_runtime.h>

#include "form_io.hpp"

using namespace cofhe;

// The kernels have external linkage so that the build can compile this file in several parallel
// passes (-DCOFHE_PART=0|1|2: each pass defines a third of the kernels); without COFHE_PART every
// kernel is compiled in one translation unit.
#ifndef COFHE_PART
#define COFHE_PART (-1)
#endif
#define PART_HAS(k) (COFHE_PART < 0 || COFHE_PART == (k))
namespace cofhe_k {

// word route for common factors (qf.hpp) in the tensor-addition kernels
#ifndef COFHE_ADD_WORD_ROUTE
#define COFHE_ADD_WORD_ROUTE true
#endif

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for
#endif

__device__ __forceinline__ Ctx make_ctx(uint32_t *lds) {
    Ctx c;
    const int lane = (int)(threadIdx.x & 63);
    c.gl = lane & (G - 1);
    c.base4 = (lane & ~(G - 1)) << 2;
    c.scr = lds + (threadIdx.x / G) * SCRATCH_WORDS;
    return c;
}

// out[i] = a[i] o b[i]: the Lehmer batches of the WG_GROUPS (32) limb groups of a workgroup
// are served by its wavefront 0 (mp.hpp: euclid_run_wg).  Groups beyond n recompute
// the last item and skip the store, so every thread reaches every barrier.
// One composition per limb group (tensor addition).  Two builds of the same body: k_compose_wg leaves room for four
// workgroups per CU (128 registers per lane, 288 of the function's values spilled; 266 before M1 and M2 came from low-half
// products, 305 with them, qf.hpp: that second route cost registers and 38 KB of code and still saved 3.4 % of the launch,
// profiles/r05_low_half/; the one-plane a', b' and the low-half c' gave 34 of them back, cost 23 KB more and saved another
// 4.4 %, profiles/r16_one_plane/; M1 and M2 from one paired division, mp_divexact without high limbs over one plane and the
// square from every chunk pair once left the spills where they were, 271 -> 268, and the code 18 KB smaller: the launch
// figures of both builds are in profiles/r17_paired_div/; r = y1 m mod a1 from the remainder-only division, mp.hpp:
// mp_rem_norm, took 268 -> 288 with the scratch frame 308 -> 316 bytes and the code 0.6 KB larger, k_add_ct 357 -> 339, the
// three-per-CU builds unchanged; the launch figures of both builds are in profiles/r18_rem_norm/) -- the form for grids of many residency
// rounds and for the 1024 workgroups of a 128x128 launch, which fill the chip exactly once; k_compose_wg3 asks for three
// (168 registers, 131 spills; 98 before the paired division) and is 6-9 % faster per workgroup, which pays whenever the whole grid is resident at three per
// CU anyway: launches of up to 768 workgroups, 24 576 compositions (64x64: 0.255 -> 0.239 ms, 110x111: 0.316 -> 0.288 ms;
// at 1024 workgroups it needs a second round: 0.49 ms.  profiles/r04_a/sizes_wps234.txt; two per CU, no spills at all, is no
// faster than three).
__device__ __forceinline__ void compose_wg_body(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n,
                                                const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_GROUPS * SCRATCH_WORDS + WG_MAIL_WORDS];
    Ctx c = make_ctx(lds);
    c.wg_mail = lds + WG_GROUPS * SCRATCH_WORDS;
    c.wg_scr0 = lds;
    c.gi = (int)(threadIdx.x / G);
    // rotate the serving wavefront over the workgroups so that the serial phases of co-resident
    // workgroups do not pile up on one SIMD: wave index 0 <=> the server
    c.wave = (int)(((threadIdx.x >> 6) + blockIdx.x) % (WG_BLOCK / 64));
    c.rank = gridDim.x <= NUM_CUS * 4 ? (int)((blockIdx.x / NUM_CUS) & 3u) : -1;
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < n ? g0 : n - 1;
#ifdef COFHE_WG_TIMING          // tools/wg_timing.hip: start / end time and placement of every workgroup
    if (threadIdx.x == 0) {
        g_wg_t[blockIdx.x * 4 + 0] = wall_clock64();
        g_wg_clk[blockIdx.x * 2 + 0] = __builtin_amdgcn_s_memtime();                  // shader-clock ticks (s_memtime)
        g_wg_t[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID
        g_wg_t[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_getreg((31 << 11) | 20);     // HW_REG_XCC_ID
    }
    if ((threadIdx.x & 63) == 0)
        g_wg_wave[blockIdx.x * 4 + (threadIdx.x >> 6)] = (__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0x0FFFFFFFu) | ((unsigned)c.wave << 28);
#endif
    QForm x, y, r;
    qf_load(c, x, a + g * REC_WORDS);
    qf_load(c, y, b + g * REC_WORDS);
    qf_compose<true, COFHE_ADD_WORD_ROUTE>(c, r, x, y, dd);
    if (g0 < n) qf_store(c, r, out + g * REC_WORDS);
#ifdef COFHE_WG_TIMING
    __syncthreads();
    if (threadIdx.x == 0) {
        g_wg_t[blockIdx.x * 4 + 1] = wall_clock64();
        g_wg_clk[blockIdx.x * 2 + 1] = __builtin_amdgcn_s_memtime();
    }
#endif
}
#if PART_HAS(0)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_compose_wg(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                                    uint32_t *__restrict__ out, uint64_t n,
                                                                    const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    compose_wg_body(a, b, out, n, absdelta, half_dbits, status);
}
#endif
#if PART_HAS(1)
__global__ void __launch_bounds__(WG_BLOCK, 3) k_compose_wg3(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                             uint32_t *__restrict__ out, uint64_t n,
                                                             const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    compose_wg_body(a, b, out, n, absdelta, half_dbits, status);
}
#endif

// Validation of form records that come from outside (wire format): reduced, primitive forms of the context's discriminant,
// clause by clause in qf.hpp (qf_form_faults).  The arithmetic assumes exactly this of its inputs; a record that fails any
// clause sets CF_ST_BAD_FORM in err.  One limb group per record: load, call, report.
#if PART_HAS(0)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_validate_forms(const uint32_t *__restrict__ recs, uint64_t n,
                                                                        const uint32_t *__restrict__ absdelta, uint32_t *__restrict__ err) {
    __shared__ uint32_t lds[WG_GROUPS * SCRATCH_WORDS];
    Ctx c = make_ctx(lds);
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    if (g0 >= n) return;
    QForm f;
    qf_load(c, f, recs + g0 * REC_WORDS);
    const uint32_t bad = qf_form_faults(c, f, absdelta);
    if (bad != 0 && c.gl == 0) atomicOr(err, CF_ST_BAD_FORM);
}
#endif

// ------------------------------------------------------------------------------------------
// Sequence kernels (powering ladders, table building, the matrix product, decryption): every limb
// group runs its own chain of compositions.  All 32 groups of a workgroup advance in lockstep,
// one qf_compose<true> per round, so that the Lehmer batches can be served by one wavefront
// (mp.hpp: euclid_run_wg): a group whose chain has ended (or which lies beyond the work size)
// squares a stand-in form and drops the result until __syncthreads_or says everybody is done.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ Ctx make_wg_ctx(uint32_t *lds) {
    Ctx c = make_ctx(lds);
    c.wg_mail = lds + WG_GROUPS * SCRATCH_WORDS;
    c.wg_scr0 = lds;
    c.gi = (int)(threadIdx.x / G);
    c.wave = (int)(((threadIdx.x >> 6) + blockIdx.x) % (WG_BLOCK / 64));
    c.rank = gridDim.x <= NUM_CUS * 4 ? (int)((blockIdx.x / NUM_CUS) & 3u) : -1;
    return c;
}
#define WG_LDS_WORDS (WG_GROUPS * SCRATCH_WORDS + WG_MAIL_WORDS)

// one lockstep round: has -> result = lhs o rhs; an idle group squares the stand-in form stored at
// `dummy_rec` (loaded on the spot: a form kept in registers for this costs 20 VGPRs of spills)
#define WG_ROUND(has, lhs, rhs, dummy_rec, result)                \
    {                                                             \
        QForm l_, r_;                                             \
        if (has) {                                                \
            l_ = (lhs);                                           \
            r_ = (rhs);                                           \
        } else {                                                  \
            qf_load(c, l_, (dummy_rec));                          \
            r_ = l_;                                              \
        }                                                         \
        qf_compose<true, false, false>(c, result, l_, r_, dd);                  \
    }

// out[g] = base[g * base_stride]^exp[...]  (binary ladder; exponent 0 -> principal form, negative ->
// inverse).  exp_mode 0: exp[g / 2] (both forms of ciphertext g / 2, base_stride 1); 1: exp[g];
// 2: exp[0] for every item (a secret-key share applied to the c1 of each ciphertext, base_stride 2)
#if PART_HAS(1)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_pow(const uint32_t *__restrict__ base, const uint32_t *__restrict__ exps,
                                                             uint32_t *__restrict__ out, uint64_t n_records,
                                                             uint32_t base_stride, uint32_t exp_mode,
                                                             const uint32_t *__restrict__ one_rec,
                                                             const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < n_records;
    const uint64_t g = alive ? g0 : n_records - 1;
    const uint32_t *e = exps + (exp_mode == 0 ? (g >> 1) : exp_mode == 1 ? g : 0) * EXP_REC_WORDS;
    // Neither the base nor the running power is kept in registers across the compositions: a form that is live across
    // the ~55 k instructions of qf_compose is spilled to scratch anyway, and the state machine around it cost 300
    // spilled registers.  The power lives in the item's OUTPUT record (which therefore must not overlap the bases: the
    // launchers see to that), a multiplication round reloads the base, an idle group squares its base and drops the result.
    const uint32_t *xrec = base + g * base_stride * REC_WORDS;
    uint32_t *accp = out + g * REC_WORDS;
    bool x_bneg, inv_bneg;            // sign of b in x and in x^-1 (signed-digit ladder, qf.hpp)
    {
        QForm x;
        qf_load(c, x, xrec);
        x_bneg = x.bneg;
        if (alive) qf_store(c, x, accp);
        qf_inverse(c, x);
        inv_bneg = x.bneg;
    }
    const int nb = exp_bitlen(e);
    const uint64_t naf = exp_naf_prepare(e);
    int t = nb == 0 ? -1 : exp_naf_top(e, naf, nb) - 1;
    bool mul_phase = false;
    while (true) {
        const bool has = alive && t >= 0;
        if (!__syncthreads_or(has ? 1 : 0)) break;
        const int dgt = has ? exp_naf_digit(e, naf, t) : 0;
        QForm l_, rhs, r;
        qf_load(c, l_, has ? (const uint32_t *)accp : xrec);
        if (has && mul_phase) {
            qf_load(c, rhs, xrec);
            rhs.bneg = dgt < 0 ? inv_bneg : x_bneg;
        } else {
            rhs = l_;
        }
        qf_compose<true, false, false>(c, r, l_, rhs, dd);
        if (has) {
            qf_store(c, r, accp);
            if (!mul_phase && dgt != 0) {
                mul_phase = true;
            } else {
                mul_phase = false;
                t--;
            }
        }
    }
    if (!alive) return;
    if (nb == 0 || e[EXP_MAG_WORDS]) {
        QForm acc;
        qf_load(c, acc, nb == 0 ? one_rec : (const uint32_t *)accp);
        if (e[EXP_MAG_WORDS]) qf_inverse(c, acc);
        qf_store(c, acc, accp);
    }
}
#endif

// ---- ciphertext-level addition with the shared first component folded -------------------------------------------
// encrypt_tensor draws ONE r per tensor (cpu_cryptosystem_tensor_ops.inl:7-12), so every ciphertext of an encrypted
// tensor carries the same c1 = h^r -- and so does every sum of such tensors.  Adding two of them element by element
// repeats the composition c1 o c1' E times.  k_c1_distinct finds out (one pass over the c1 records, ~20 us at
// 128x128); k_add_ct then runs E + 1 compositions instead of 2 E and k_c1_spread copies the one c1 result into every
// ciphertext.  Tensors whose c1 differ (results of scal_ciphertext_tensors, mixed sources) take the plain path; the
// records written are the same either way.
#if PART_HAS(2)
__global__ void k_c1_distinct(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint64_t n_ct, uint32_t *__restrict__ flag) {
    const uint64_t words = n_ct * REC_WORDS;
    bool diff = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t ct = i / REC_WORDS, w = i % REC_WORDS;
        const uint64_t at = ct * 2 * REC_WORDS + w;
        diff |= (a[at] != a[w]) | (b[at] != b[w]);
    }
    if (__builtin_amdgcn_ballot_w64(diff) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
__global__ void k_c1_spread(uint32_t *__restrict__ out, uint64_t n_ct, const uint32_t *__restrict__ flag) {
    if (*flag) return;
    const uint64_t words = n_ct * REC_WORDS;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + REC_WORDS; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t ct = i / REC_WORDS, w = i % REC_WORDS;
        out[ct * 2 * REC_WORDS + w] = out[w];
    }
}
// recs[i] = recs[0], i < n (one form per element: the partial decryptions of a tensor whose c1 are shared)
__global__ void k_spread_records(uint32_t *__restrict__ recs, uint64_t n) {
    const uint64_t words = n * REC_WORDS;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + REC_WORDS; i < words; i += (uint64_t)gridDim.x * blockDim.x)
        recs[i] = recs[i % REC_WORDS];
}
__device__ __forceinline__ void add_ct_body(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n_ct,
                                            const uint32_t *__restrict__ flag, const uint32_t *__restrict__ absdelta, int half_dbits,
                                            uint32_t *__restrict__ status, uint32_t only) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    const uint32_t distinct = *flag;
    // only: 0 this launch does the addition whatever the flag says; 1 / 2: it is one of a pair of launches and acts when the
    // tensors share their c1 / when they do not (the other launch of the pair returns at once)
    if (only != 0 && (only == 1) != (distinct == 0)) return;
    // compositions of this launch: every record, or the c2 of every ciphertext plus the one shared c1
    const uint64_t n = distinct ? 2 * n_ct : n_ct + 1;
    if ((uint64_t)blockIdx.x * WG_GROUPS >= n) return;           // whole workgroups only: nobody is left at a barrier
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < n ? g0 : n - 1;
    const uint64_t rec = distinct ? g : (g < n_ct ? 2 * g + 1 : 0);
    QForm x, y, r;
    qf_load(c, x, a + rec * REC_WORDS);
    qf_load(c, y, b + rec * REC_WORDS);
    qf_compose<true, COFHE_ADD_WORD_ROUTE>(c, r, x, y, dd);
    if (g0 < n) qf_store(c, r, out + rec * REC_WORDS);
}
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_add_ct(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                                uint32_t *__restrict__ out, uint64_t n_ct, const uint32_t *__restrict__ flag,
                                                                const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status, uint32_t only) {
    add_ct_body(a, b, out, n_ct, flag, absdelta, half_dbits, status, only);
}
// three workgroups per CU (see k_compose_wg3): for grids of at most 768 workgroups
__global__ void __launch_bounds__(WG_BLOCK, 3) k_add_ct3(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                         uint32_t *__restrict__ out, uint64_t n_ct, const uint32_t *__restrict__ flag,
                                                         const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status, uint32_t only) {
    add_ct_body(a, b, out, n_ct, flag, absdelta, half_dbits, status, only);
}
#endif

// table[j] = base^(2^j), j < len: one chain of squarings (every group of the one workgroup runs it in lockstep so
// that the served Euclid has its 32 requests; group 0 stores).  Built once per base and cached by the context.
#if PART_HAS(1)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_square_chain(const uint32_t *__restrict__ base, uint32_t *__restrict__ table, uint32_t len,
                                                                      const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const bool writer = (threadIdx.x / G) == 0 && blockIdx.x == 0;
    QForm acc;
    qf_load(c, acc, base);
    if (writer) qf_store(c, acc, table);
    for (uint32_t j = 1; j < len; j++) {
        QForm r;
        qf_compose<true, false, false>(c, r, acc, acc, dd);
        acc = r;
        if (writer) qf_store(c, acc, table + (uint64_t)j * REC_WORDS);
    }
}
// out[i] = tabs[(idx[i] >> 24) & 0x7F][idx[i] & 0xFFFFFF], inverted when bit 31 of idx[i] is set; idx[i] == 0xFFFFFFFF:
// the principal form.  The entries of the product trees: table forms (fixed-base powers) selected by signed digits.
__global__ void k_gather_signed(const uint64_t *__restrict__ tabs, const uint32_t *__restrict__ idx, uint64_t n,
                                const uint32_t *__restrict__ one_rec, uint32_t *__restrict__ out) {
    __shared__ uint32_t lds[WG_GROUPS * SCRATCH_WORDS];
    Ctx c = make_ctx(lds);
    const uint64_t g = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    if (g >= n) return;
    const uint32_t ix = idx[g];
    // padding entries (0xFFFFFFFF) name no table: the table pointer is only read for real entries
    const uint32_t *src = one_rec;
    if (ix != 0xFFFFFFFFu) src = (const uint32_t *)(uintptr_t)tabs[(ix >> 24) & 0x7Fu] + (uint64_t)(ix & 0xFFFFFFu) * REC_WORDS;
    QForm f;
    qf_load(c, f, src);
    if (ix != 0xFFFFFFFFu && (ix >> 31)) qf_inverse(c, f);
    qf_store(c, f, out + g * REC_WORDS);
}
// Encryption, step 1: the entries of f^(m_i) o pk^r for every plaintext, entry-major ([slot][element], so that the
// pairwise product tree below walks k_compose_pairs' [m][q] layout with q = elements): slot 0 is pk^r (table 1,
// record 1), then one entry f^(+-2^j) (table 0, record 2 j: the decryption table holds f^(-2^j)) per non-zero signed
// digit of m_i mod 2^k, the rest principal forms.  cap slots per element; the largest count goes to *max_slots.
__global__ void k_encrypt_select(const uint32_t *__restrict__ plain, uint64_t n_ct, int kbits, uint32_t cap, uint32_t *__restrict__ idx,
                                 uint32_t *__restrict__ max_slots) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ct) return;
    const uint32_t *e = plain + i * EXP_REC_WORDS;
    const bool neg = e[EXP_MAG_WORDS] != 0;              // f^(-|m|): every digit changes sign
    const uint64_t naf = exp_naf_prepare(e);
    uint32_t slot = 0;
    idx[(uint64_t)slot++ * n_ct + i] = (1u << 24) | 1u;
    for (int j = 0; j < kbits && slot < cap; j++) {
        const int dgt = exp_naf_digit(e, naf, j);
        if (dgt != 0) idx[(uint64_t)slot++ * n_ct + i] = (uint32_t)(2 * j) | (((dgt > 0) != neg) ? 0x80000000u : 0u);
    }
    atomicMax(max_slots, slot);
    for (; slot < cap; slot++) idx[(uint64_t)slot * n_ct + i] = 0xFFFFFFFFu;
}
// out[2 i] = c1, out[2 i + 1] = c2[i]
__global__ void k_zip_ciphertexts(const uint32_t *__restrict__ c1, const uint32_t *__restrict__ c2, uint64_t n_ct, uint32_t *__restrict__ out) {
    const uint64_t words = n_ct * 2 * REC_WORDS;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t rec = i / REC_WORDS, w = i % REC_WORDS;
        out[i] = (rec & 1) ? c2[(rec >> 1) * REC_WORDS + w] : c1[w];
    }
}
#endif

// One level of the pairwise product tree of the accumulation below, for outputs too few to fill the GPU
// with chains: x is [n][m][q] forms (q = 2p, a row of the matrix of element products), out is
// [n][ceil(m/2)][q] with out[i][jj][.] = x[i][2jj][.] o x[i][2jj+1][.]; an unpaired last slice is composed
// with `pad` (the principal form, or -- on the last level, m == 1 -- the Enc(0) the sum starts from:
// then pad is indexed by h = q & 1 and out[i][0][.] = x[i][0][.] o zero[h]).
#if PART_HAS(0)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_compose_pairs(const uint32_t *__restrict__ x, const uint32_t *__restrict__ pad,
                                                                       uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t q,
                                                                       uint32_t pad_by_h, const uint32_t *__restrict__ absdelta,
                                                                       int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint32_t mh = (m + 1) / 2;
    const uint64_t total = (uint64_t)n * mh * q;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < total ? g0 : total - 1;
    const uint32_t qq = (uint32_t)(g % q);
    const uint64_t ij = g / q;
    const uint32_t jj = (uint32_t)(ij % mh), i = (uint32_t)(ij / mh);
    const uint64_t ia = ((uint64_t)i * m + 2 * jj) * q + qq;
    const bool paired = 2 * jj + 1 < m;
    QForm a, b, r;
    qf_load(c, a, x + ia * REC_WORDS);
    qf_load(c, b, paired ? x + (ia + q) * REC_WORDS : pad + (pad_by_h ? (qq & 1u) : 0u) * REC_WORDS);
    // Slices are padded with principal forms (a = 1) to a common length, and a product with the principal form is the
    // other operand: when no group of the workgroup has two proper operands the round of compositions is skipped
    // (in the entry-major layout of the encryption tree the padding of 32 neighbouring elements lines up).
    const bool a_one = mp_is_word(c, a.a, 1), b_one = mp_is_word(c, b.a, 1);
    if (!__syncthreads_or((a_one || b_one) ? 0 : 1)) {
        if (g0 < total) qf_store(c, a_one ? b : a, out + g * REC_WORDS);
        return;
    }
    qf_compose<true, false, false>(c, r, a, b, dd);
    if (g0 < total) qf_store(c, r, out + g * REC_WORDS);
}
#endif

// out[(i*p+k)*2+h] = zero[h] o prod_j x[((i*m+j)*p+k)*2+h]: the accumulation loop of the
// ciphertext x ciphertext matrix product (SMPCCipherTextMultiplier, include/smpc/
// ciphertext_multiplications.hpp:85-101: res[i,k] starts as a copy of Enc(0) and absorbs the m
// element products res_nmp[i,j,k]).  One limb group per output form, m compositions each.
#if PART_HAS(0)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_accumulate(const uint32_t *__restrict__ x, const uint32_t *__restrict__ zero,
                                                                    uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t p,
                                                                    const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t total = (uint64_t)n * p * 2;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < total;
    const uint64_t g = alive ? g0 : total - 1;
    const uint32_t h = (uint32_t)(g & 1);
    const uint64_t ik = g >> 1;
    const uint32_t i = (uint32_t)(ik / p), k = (uint32_t)(ik % p);
    // the running product lives in the output record (see k_pow); idle groups recompute zero o x and store nothing
    uint32_t *accp = out + g * REC_WORDS;
    for (uint32_t j = 0; j < m; j++) {          // same trip count for every group: barriers line up
        QForm l_, rhs, r;
        qf_load(c, l_, (j == 0 || !alive) ? zero + h * REC_WORDS : (const uint32_t *)accp);
        qf_load(c, rhs, x + ((((uint64_t)i * m + j) * p + k) * 2 + h) * REC_WORDS);
        qf_compose<true, false, false>(c, r, l_, rhs, dd);
        if (alive) qf_store(c, r, accp);
    }
    if (m == 0 && alive) {
        QForm z;
        qf_load(c, z, zero + h * REC_WORDS);
        qf_store(c, z, accp);
    }
}
#endif

// ------------------------------------------------------------------------------------------
// Plaintext-matrix x ciphertext-matrix product, out[i,k] = zero o prod_j cts[i,j]^s[j,k]
// (reference: scal_ciphertext_tensors 2-D, cpu_cryptosystem_tensor_ops.inl:342-461, whose
// qfi_nupow -- include/x86_64/qfi.inl:1-135 -- is a width-7 wNAF with a table of odd powers per
// base shared by the p exponents of a row).  Here: (1) k_wnaf_digits recodes every exponent into
// width-w non-adjacent form, one signed byte per bit position, laid out [position][j*p+k];
// (2) k_pow_table builds the odd powers x, x^3, ..., x^(2^(w-1)-1) of every base in HBM
// (w = 8: 64 entries = 43 KB per base, 5.6 GB for a 256x256 operand -- 288 GB are there to be
// used); (3) k_scal_matmul_wnaf runs ONE squaring chain per output coefficient (Straus) and, at
// each bit position, one composition per non-zero digit of the column: bits/(w+1) per base on
// average, and negative weights (2^k - |x| after make_plaintext) cost what |x| costs.
// ------------------------------------------------------------------------------------------

// longest exponent of a plaintext tensor (the host picks the window width from it)
#if PART_HAS(0)
__global__ void k_exp_maxbits(const uint32_t *__restrict__ exps, uint64_t n_exps, uint32_t *__restrict__ maxbits) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_exps) return;
    const int nb = exp_bitlen(exps + idx * EXP_REC_WORDS);
    if (nb) atomicMax(maxbits, (uint32_t)nb);
}
#endif

#if PART_HAS(0)
__global__ void k_wnaf_digits(const uint32_t *__restrict__ exps, uint64_t n_exps, uint32_t w, int8_t *__restrict__ digits,
                              uint32_t *__restrict__ maxlen) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_exps) return;
    const uint32_t *e = exps + idx * EXP_REC_WORDS;
    const bool neg = e[EXP_MAG_WORDS] != 0;
    const int nb = exp_bitlen(e);
    const uint32_t mask = (1u << w) - 1u, half = 1u << (w - 1);
    int t = 0;
    uint32_t carry = 0;
    uint32_t len = 0;
    while (t < nb || carry) {
        const uint32_t v = (t < nb ? exp_digit(e, t, (int)w) : 0u) + carry;     // exp_digit: w <= 8 bits from position t
        if ((v & 1u) == 0) {
            // even: digit 0 (the buffer is pre-zeroed); the carry survives only through a set bit
            carry = ((t < nb ? (uint32_t)exp_bit(e, t) : 0u) + carry) >> 1;
            t++;
            continue;
        }
        int d;
        const uint32_t vv = v & mask;                     // v <= 2^w - 1 here (v odd)
        if (vv > half) {
            d = (int)vv - (int)(mask + 1u);
            carry = 1;
        } else {
            d = (int)vv;
            carry = 0;
        }
        digits[(uint64_t)t * n_exps + idx] = (int8_t)(neg ? -d : d);
        len = (uint32_t)t + 1;
        t += (int)w;
    }
    if (len) atomicMax(maxlen, len);
}
#endif

// table[r * tw + d] = base[r]^(2d+1), d < tw: one limb group per base
#if PART_HAS(1)
__device__ __forceinline__ void k_pow_table_body(const uint32_t *__restrict__ base, uint32_t *__restrict__ table,
                                                                   uint64_t n_records, uint32_t tw,
                                                                   const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < n_records;
    const uint64_t g = alive ? g0 : n_records - 1;
    // No form stays in registers across a composition (see k_pow): x^2 is parked in the LAST slot of the base's table
    // until the last product overwrites it, every other round reads the previous entry and writes the next.
    //   d = 0:  slot tw-1 <- x o x;   d >= 1:  slot d <- slot d-1 o slot tw-1   (d = tw-1 reads x^2 before it stores)
    uint32_t *out = table + g * tw * REC_WORDS;
    {
        QForm x;
        qf_load(c, x, base + g * REC_WORDS);
        if (alive) qf_store(c, x, out);
    }
    if (tw == 1) return;                               // uniform over the grid
    // idle groups (beyond n_records) square the last base every round and store nothing (the table of that base is
    // being written by its own group: not theirs to read)
    for (uint32_t d = 0; d < tw; d++) {               // same trip count for every group: no vote needed
        QForm l_, r_, r;
        if (d == 0 || !alive) {
            qf_load(c, l_, base + g * REC_WORDS);
            r_ = l_;
        } else {
            qf_load(c, l_, out + (uint64_t)(d - 1) * REC_WORDS);
            qf_load(c, r_, out + (uint64_t)(tw - 1) * REC_WORDS);
        }
        qf_compose<true, false, false>(c, r, l_, r_, dd);
        if (alive) qf_store(c, r, out + (uint64_t)(d == 0 ? tw - 1 : d) * REC_WORDS);
    }
}
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_pow_table(const uint32_t *__restrict__ base, uint32_t *__restrict__ table,
                                                                   uint64_t n_records, uint32_t tw,
                                                                   const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    k_pow_table_body(base, table, n_records, tw, absdelta, half_dbits, status);
}
// three workgroups per CU (see k_compose_wg3): for grids of at most 768 workgroups
__global__ void __launch_bounds__(WG_BLOCK, 3) k_pow_table3(const uint32_t *__restrict__ base, uint32_t *__restrict__ table,
                                                                   uint64_t n_records, uint32_t tw,
                                                                   const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    k_pow_table_body(base, table, n_records, tw, absdelta, half_dbits, status);
}
#endif

// The schedule of a column of the product: the compositions of out[., seg, k, .] in order, one op word each (layout.hpp).  It depends
// on the digits of the column only -- not on the row i or the form h -- so it is worked out ONCE per column here (one
// thread per column walks the digit matrix: bit positions from the top, one squaring slot per position, then the bases
// of the segment with a non-zero digit) instead of by every chain in every round (until round 3 each round's scan for the
// next non-zero digit was a chain of dependent byte loads in front of the table gather).
// word route for common factors (qf.hpp) in the matrix product: 248.2 vs 252.8 ms at 64 x 256 . 256 x 256, interleaved runs
#ifndef COFHE_MATMUL_WORD_ROUTE
#define COFHE_MATMUL_WORD_ROUTE true
#endif
#if PART_HAS(0)
__global__ void k_matmul_schedule(const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen, uint32_t m, uint32_t p,
                                  uint32_t segs, uint32_t rcap, uint32_t *__restrict__ ops, uint32_t *__restrict__ counts,
                                  uint32_t *__restrict__ status) {
    // one wavefront per column: 64 bases of a bit position at a time, compacted in order with a ballot
    const uint32_t col = blockIdx.x;                                       // seg * p + k
    const uint32_t lane = threadIdx.x;
    const uint32_t k = col % p, seg = col / p;
    const uint32_t seglen = (m + segs - 1) / segs;
    const uint32_t j0 = seg * seglen, j1 = (j0 + seglen < m) ? j0 + seglen : m;
    const uint64_t n_exps = (uint64_t)m * p;
    uint32_t *o = ops + (uint64_t)col * rcap;
    uint32_t r = 0;                                                        // wave-uniform
    bool have = false;
    for (int t = (int)*maxlen - 1; t >= 0; t--) {
        if (have) {
            if (lane == 0 && r < rcap) o[r] = MM_SQUARE << 29;
            r++;
        }
        const int8_t *row = digits + (uint64_t)t * n_exps + k;
        for (uint32_t jb = j0; jb < j1; jb += 64) {
            const uint32_t j = jb + lane;
            const int dg = j < j1 ? (int)row[(uint64_t)j * p] : 0;
            const uint64_t mask = __builtin_amdgcn_ballot_w64(dg != 0);
            if (dg != 0) {
                const uint32_t before = (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
                const uint32_t mag = (uint32_t)(dg < 0 ? -dg : dg);
                const bool first = !have && before == 0;
                if (r + before < rcap)
                    o[r + before] = ((first ? MM_FIRST : MM_MUL) << 29) | (j << 8) | (dg < 0 ? 0x80u : 0u) | (mag >> 1);
            }
            r += (uint32_t)__builtin_popcountll(mask);
            have = have || mask != 0;
        }
    }
    if (segs == 1) {
        if (lane == 0 && r < rcap) o[r] = (have ? MM_ZEROMUL : MM_FIRSTZERO) << 29;
        r++;
    } else if (!have) {
        if (lane == 0 && r < rcap) o[r] = MM_FIRSTONE << 29;
        r++;
    }
    if (lane == 0) {
        counts[col] = r < rcap ? r : rcap;
        // rcap is the worst case of the digits k_wnaf_digits wrote (exp_bits and maxlen come from two kernels): a list that
        // does not fit means they disagree -- the chain would be truncated and the product wrong, so say so
        if (r > rcap) atomicOr(status, CF_ST_SCHEDULE_CAP);
    }
}
#endif

#if PART_HAS(2)
__device__ __forceinline__ void k_scal_matmul_wnaf_body(const uint32_t *__restrict__ table, const uint32_t *__restrict__ ops,
                                                                          const uint32_t *__restrict__ counts, uint32_t rcap,
                                                                          const uint32_t *__restrict__ zero, uint32_t *__restrict__ out,
                                                                          uint32_t n, uint32_t m, uint32_t p, uint32_t tw,
                                                                          uint32_t segs, const uint32_t *__restrict__ one_rec,
                                                                          const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    // segs == 1: out[i][k][h] = zero o prod_j ...; segs > 1 (few outputs): the inner dimension is cut into
    // `segs` ranges with a squaring chain each, out[i][seg][k][h] = prod_{j in range} ... without the zero;
    // the partial products are then folded by the accumulation tree (k_compose_pairs)
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t total = (uint64_t)n * segs * p * 2;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < total;
    const uint64_t g = alive ? g0 : total - 1;
    // chains are numbered column-major, g = ((seg p + k) n + i) 2 + h: the schedule of a chain depends on (seg, k) only,
    // so the 32 chains of a workgroup (16 rows x 2 forms of ONE column whenever 2 n is a multiple of 32) do the same
    // number of compositions at every bit position and the lockstep rounds carry no padding (numbered row-major, 16
    // columns per workgroup, every round waited for the busiest of 16 schedules)
    const uint32_t h = (uint32_t)(g & 1);
    const uint64_t ci = g >> 1;
    const uint32_t i = (uint32_t)(ci % n);
    const uint32_t col = (uint32_t)(ci / n);
    const uint32_t k = col % p, seg = col / p;
    // The running product lives in the chain's OUTPUT record, not in registers: a round loads it, composes and stores
    // it back.  A form kept live across the ~55 k instructions of qf_compose is spilled to scratch anyway (20 VGPRs and
    // the state machine around them: 520 spilled registers in round 2); through the record the compiler only carries
    // the scalars of the state machine.  672 B out and back per round against ~400 us of arithmetic.
    // (a chain-major scratch array for the running products -- 32 consecutive records per workgroup instead of records a
    // whole output row apart -- measured no different: 247.8 vs 248.1 ms at 64 x 256 . 256 x 256)
    uint32_t *accp = out + ((((uint64_t)i * segs + seg) * p + k) * 2 + h) * REC_WORDS;
    const uint32_t *dummy = zero + h * REC_WORDS;
    const uint32_t *myops = ops + (uint64_t)col * rcap;
    const uint32_t nops = alive ? counts[col] : 0u;
    uint32_t r = 0;
    while (true) {
        // this chain's next composition (if any): rsrc = record of the right-hand side (nullptr: the running product
        // itself, a squaring), rinv = take its inverse.  The first entry of a chain becomes the running product as it is.
        const uint32_t *rsrc = nullptr;
        bool rinv = false, has = false;
        while (r < nops && !has) {
            const uint32_t op = myops[r++];
            const uint32_t kind = op >> 29;
            const uint32_t *ent = table + ((((uint64_t)i * m + ((op >> 8) & 0x1FFFFFu)) * 2 + h) * tw + (op & 0x7Fu)) * REC_WORDS;
            if (kind == MM_FIRST || kind == MM_FIRSTZERO || kind == MM_FIRSTONE) {
                QForm f;
                qf_load(c, f, kind == MM_FIRST ? ent : kind == MM_FIRSTZERO ? dummy : one_rec);
                if (kind == MM_FIRST && (op & 0x80u)) qf_inverse(c, f);
                qf_store(c, f, accp);
            } else {
                has = true;
                if (kind == MM_MUL) {
                    rsrc = ent;
                    rinv = (op & 0x80u) != 0;
                } else if (kind == MM_ZEROMUL) {
                    rsrc = dummy;
                }
            }
        }
        if (!__syncthreads_or(has ? 1 : 0)) break;
        QForm l_, r_, r2;
        qf_load(c, l_, has ? (const uint32_t *)accp : dummy);
        if (has && rsrc) {
            qf_load(c, r_, rsrc);
            if (rinv) qf_inverse(c, r_);
        } else {
            r_ = l_;
        }
        qf_compose<true, COFHE_MATMUL_WORD_ROUTE, false>(c, r2, l_, r_, dd);
        if (has) qf_store(c, r2, accp);
    }
}
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_scal_matmul_wnaf(const uint32_t *__restrict__ table, const uint32_t *__restrict__ ops,
                                                                          const uint32_t *__restrict__ counts, uint32_t rcap,
                                                                          const uint32_t *__restrict__ zero, uint32_t *__restrict__ out,
                                                                          uint32_t n, uint32_t m, uint32_t p, uint32_t tw,
                                                                          uint32_t segs, const uint32_t *__restrict__ one_rec,
                                                                          const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    k_scal_matmul_wnaf_body(table, ops, counts, rcap, zero, out, n, m, p, tw, segs, one_rec, absdelta, half_dbits, status);
}
// three workgroups per CU (see k_compose_wg3): for grids of at most 768 workgroups
__global__ void __launch_bounds__(WG_BLOCK, 3) k_scal_matmul_wnaf3(const uint32_t *__restrict__ table, const uint32_t *__restrict__ ops,
                                                                          const uint32_t *__restrict__ counts, uint32_t rcap,
                                                                          const uint32_t *__restrict__ zero, uint32_t *__restrict__ out,
                                                                          uint32_t n, uint32_t m, uint32_t p, uint32_t tw,
                                                                          uint32_t segs, const uint32_t *__restrict__ one_rec,
                                                                          const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    k_scal_matmul_wnaf_body(table, ops, counts, rcap, zero, out, n, m, p, tw, segs, one_rec, absdelta, half_dbits, status);
}
#endif

// ------------------------------------------------------------------------------------------
// The matrix product as a PRODUCT TREE (round 4).  out[i,k] = zero o prod_t (P[k,t][i])^(2^t) with
// P[k,t][i] = prod_{j : digit(j,k,t) != 0} table[i,j][|digit| >> 1]^(+-1): the per-position products P are independent of
// each other and of the squarings, so they are multiplied out as pairwise trees over ALL (column, position, row, form)
// at once -- launches of millions of independent compositions at the rate of the tensor-addition kernel -- and only the
// Horner step acc <- acc^2 o P[k,t] stays a lockstep chain (2 bits compositions per output, the existing chain kernel with
// the tree's top level as its "table").  Same number of compositions as the chains of k_scal_matmul_wnaf, which stored and
// reloaded every running product once per round and ran a column's hundreds of compositions one after the other.
//
// A SEGMENT is one (position t, column k), s = t p + k, with cnt[s] non-zero digits.  Level 0 of its tree are its table
// entries (ent0: j << 8 | negative << 7 | |digit| >> 1), level l + 1 pairs up level l: c_(l+1)[s] = ceil(c_l[s] / 2), an unpaired
// last element is copied.  off_l = exclusive scan of c_l over the segments, N_l its total, map_l[u] = segment of element u.
// The levels of a chunk of R rows live in two buffers used in turn, record index (i N_l + u) 2 + h -- row-major like a table,
// so the top level T (every c_T <= 1) is read by the Horner kernel as a table with N_T one-entry bases per row.
// ------------------------------------------------------------------------------------------
#if PART_HAS(0)
// cnt[s] = number of non-zero digits of column k at position t, s = t p + k < len p
__global__ void k_tree_count(const int8_t *__restrict__ digits, const uint32_t *__restrict__ maxlen, uint32_t m, uint32_t p,
                             uint32_t *__restrict__ cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (uint64_t)*maxlen * p) return;
    const uint32_t t = (uint32_t)(s / p), k = (uint32_t)(s % p);
    const int8_t *row = digits + (uint64_t)t * m * p + k;
    uint32_t c = 0;
    for (uint32_t j = 0; j < m; j++) c += row[(uint64_t)j * p] != 0 ? 1u : 0u;
    cnt[s] = c;
}
// ONE workgroup: c_l, off_l (exclusive scans over the S = len p segments) and N_l for every level, and the top level T.
// c and off hold TREE_LEVELS + 1 rows of S_cap and S_cap + 1 words; info = [N_0 .. N_TREE_LEVELS, T, S].
__global__ void __launch_bounds__(1024) k_tree_plan(const uint32_t *__restrict__ maxlen, uint32_t p, uint32_t S_cap, uint32_t *__restrict__ c,
                                                    uint32_t *__restrict__ off, uint32_t *__restrict__ info) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t s_max;
    const uint32_t S = *maxlen * p;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t per = (S + nt - 1) / nt;
    const uint32_t lo = tid * per < S ? tid * per : S, hi = lo + per < S ? lo + per : S;
    uint32_t top = TREE_LEVELS;
    for (int l = 0; l <= TREE_LEVELS; l++) {
        uint32_t *cl = c + (uint64_t)l * S_cap, *ol = off + (uint64_t)l * (S_cap + 1);
        if (tid == 0) s_max = 0;
        __syncthreads();
        uint32_t sum = 0, mx = 0;
        for (uint32_t s = lo; s < hi; s++) {
            uint32_t v = cl[s];
            if (l > 0) {
                v = (c[(uint64_t)(l - 1) * S_cap + s] + 1) / 2;
                cl[s] = v;
            }
            sum += v;
            mx = v > mx ? v : mx;
        }
        part[tid] = sum;
        atomicMax(&s_max, mx);
        __syncthreads();
        if (tid == 0) {                              // 1024 partial sums: a serial scan is a few microseconds
            uint32_t run = 0;
            for (uint32_t i = 0; i < nt; i++) {
                const uint32_t v = part[i];
                part[i] = run;
                run += v;
            }
            info[l] = run;
            ol[S] = run;
        }
        __syncthreads();
        uint32_t run = part[tid];
        for (uint32_t s = lo; s < hi; s++) {
            ol[s] = run;
            run += cl[s];
        }
        if (l >= 1 && s_max <= 1 && top == TREE_LEVELS) top = (uint32_t)l;     // at least one level: the top must be a buffer
        __syncthreads();
    }
    if (tid == 0) {
        info[TREE_LEVELS + 1] = top;
        info[TREE_LEVELS + 2] = S;
    }
}
// level-0 entries of every segment (one wavefront per segment, the non-zero digits compacted in order of j) and the
// element -> segment maps of levels 1 .. T (maps of the levels one after the other: base of level l = N_1 + .. + N_(l-1))
__global__ void k_tree_fill(const int8_t *__restrict__ digits, uint32_t m, uint32_t p, uint32_t S_cap, const uint32_t *__restrict__ c,
                            const uint32_t *__restrict__ off, const uint32_t *__restrict__ info, uint32_t *__restrict__ ent0,
                            uint32_t *__restrict__ maps) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint32_t S = info[TREE_LEVELS + 2], T = info[TREE_LEVELS + 1];
    if (s >= S) return;
    const uint32_t t = s / p, k = s % p;
    const int8_t *row = digits + (uint64_t)t * m * p + k;
    uint32_t r = off[s];
    for (uint32_t jb = 0; jb < m; jb += 64) {
        const uint32_t j = jb + lane;
        const int dg = j < m ? (int)row[(uint64_t)j * p] : 0;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(dg != 0);
        if (dg != 0) {
            const uint32_t before = (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
            const uint32_t mag = (uint32_t)(dg < 0 ? -dg : dg);
            ent0[r + before] = (j << 8) | (dg < 0 ? 0x80u : 0u) | (mag >> 1);
        }
        r += (uint32_t)__builtin_popcountll(mask);
    }
    uint32_t base = 0;
    for (uint32_t l = 1; l <= T; l++) {
        const uint32_t cl = c[(uint64_t)l * S_cap + s], ol = off[(uint64_t)l * (S_cap + 1) + s];
        for (uint32_t q = lane; q < cl; q += 64) maps[base + ol + q] = s;
        base += info[l];
    }
}
// the Horner schedule of column k over the top level of the tree, in k_scal_matmul_wnaf's op format (the "table" being the
// top level: base index = off_T[s], one entry per base): per position a squaring and, when the segment is not empty, its product
__global__ void k_tree_horner_schedule(const uint32_t *__restrict__ maxlen, uint32_t p, uint32_t S_cap, const uint32_t *__restrict__ c,
                                       const uint32_t *__restrict__ off, const uint32_t *__restrict__ info, uint32_t rcap,
                                       uint32_t *__restrict__ ops, uint32_t *__restrict__ counts, uint32_t *__restrict__ status) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p) return;
    const uint32_t T = info[TREE_LEVELS + 1];
    const uint32_t *offT = off + (uint64_t)T * (S_cap + 1);
    uint32_t *o = ops + (uint64_t)k * rcap;
    uint32_t r = 0;
    bool have = false, big = false;
    for (int t = (int)*maxlen - 1; t >= 0; t--) {
        const uint32_t s = (uint32_t)t * p + k;
        if (have) {
            if (r < rcap) o[r] = MM_SQUARE << 29;
            r++;
        }
        if (c[s] != 0) {
            if (r < rcap) o[r] = ((have ? MM_MUL : MM_FIRST) << 29) | ((offT[s] & (MM_INDEX_LIMIT - 1)) << 8);
            r++;
            have = true;
            big = big || offT[s] >= MM_INDEX_LIMIT;
        }
    }
    if (r < rcap) o[r] = (have ? MM_ZEROMUL : MM_FIRSTZERO) << 29;
    r++;
    counts[k] = r < rcap ? r : rcap;
    // an index the op word cannot hold (the host does not take the tree then): the product would be wrong, so say so
    if (r > rcap || big) atomicOr(status, CF_ST_SCHEDULE_CAP);
}
#endif

// One level of the trees of a chunk of `rows` rows: element u of level l + 1 (segment s = map[u], q = u - off_next[s]) is the
// product of elements 2 q and 2 q + 1 of segment s at level l, or a copy of element 2 q when that is the segment's last.
// Level 0 reads table entries (src = the chunk's first table row, ent0), higher levels the previous buffer.  Work item
// g = (u, i, h), u slowest: with 2 rows a multiple of 32 the groups of a workgroup share u, so a copy is a copy for all of them
// and the workgroup skips the composition.
#if PART_HAS(2)
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_tree_level(const uint32_t *__restrict__ src, uint32_t from_table, const uint32_t *__restrict__ ent0,
                                                                    const uint32_t *__restrict__ off_cur, const uint32_t *__restrict__ off_next,
                                                                    const uint32_t *__restrict__ map_next, uint32_t n_cur, uint32_t n_next,
                                                                    uint32_t rows, uint32_t m, uint32_t tw, uint32_t *__restrict__ dst,
                                                                    const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t total = (uint64_t)n_next * rows * 2;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < total ? g0 : total - 1;
    const uint32_t ih = (uint32_t)(g % ((uint64_t)rows * 2)), u = (uint32_t)(g / ((uint64_t)rows * 2));
    const uint32_t i = ih >> 1, h = ih & 1u;
    const uint32_t sgm = map_next[u], q = u - off_next[sgm];
    const uint32_t base = off_cur[sgm], cnt = off_cur[sgm + 1] - base;
    const bool paired = 2 * q + 1 < cnt;
    QForm a, b, r;
    auto element = [&](QForm &f, uint32_t e) {
        if (from_table) {
            const uint32_t w = ent0[e];
            qf_load(c, f, src + ((((uint64_t)i * m + (w >> 8)) * 2 + h) * tw + (w & 0x7Fu)) * REC_WORDS);
            if (w & 0x80u) qf_inverse(c, f);
        } else {
            qf_load(c, f, src + (((uint64_t)i * n_cur + e) * 2 + h) * REC_WORDS);
        }
    };
    element(a, base + 2 * q);
    uint32_t *out = dst + (((uint64_t)i * n_next + u) * 2 + h) * REC_WORDS;
    if (!__syncthreads_or(paired ? 1 : 0)) {                     // a workgroup of copies
        if (g0 < total) qf_store(c, a, out);
        return;
    }
    if (paired) element(b, base + 2 * q + 1); else b = a;
    qf_compose<true, false, false>(c, r, a, b, dd);
    if (g0 < total) qf_store(c, paired ? r : a, out);
}
#endif

// out[g] = base[g * base_stride]^e for ONE exponent shared by all items (a secret key or key share
// applied to the c1 of every ciphertext: partDecrypt, cpu_cryptosystem_distributed.inl:259-269, and
// the c1^sk of decryption).  The exponent is recoded once into width-w non-adjacent form
// (k_wnaf_digits with a single exponent); every limb group builds the odd powers of its own base
// in HBM and runs the same ladder, so the whole workgroup is in lockstep by construction:
// bits squarings + bits/(w+1) table compositions + 2^(w-2) to build the table.
#if PART_HAS(1)
// WG = 1: the kernels' usual form (32 groups in lockstep, served remainder sequences).  WG = 0: the SOLO form for a handful
// of ladders -- one wavefront, every group runs its remainder sequences inside its own 8 lanes (euclid_run: no mailbox, no
// workgroup barrier, groups beyond the work size simply leave): the latency of a composition is what counts when a
// decryption is ONE ladder of ~1100 dependent compositions, and a round trip through the serving wavefront costs more
// than the 8-fold redundant batch.
template <int WG>
__device__ __forceinline__ void pow_shared_body(Ctx &c, const uint32_t *__restrict__ base, const int8_t *__restrict__ digits,
                                                const uint32_t *__restrict__ maxlen, uint32_t *__restrict__ table,
                                                uint32_t *__restrict__ out, uint64_t n_items, uint32_t base_stride,
                                                uint32_t tw, const uint32_t *__restrict__ one_rec,
                                                const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * (WG ? WG_GROUPS : 64 / G) + threadIdx.x / G;
    const bool alive = g0 < n_items;
    if (WG == 0 && !alive) return;
    const uint64_t g = alive ? g0 : n_items - 1;
    // slots 0 .. tw-1: odd powers; slot tw: x^2; slot tw+1: the running power.  Padded to the grid: idle groups own
    // slots too.  No form is kept in registers across a composition (see k_pow): every round loads its two operands
    // from the group's slots and stores the result into one.
    uint32_t *tab = table + g0 * (tw + 2) * REC_WORDS;
    uint32_t *accp = tab + (uint64_t)(tw + 1) * REC_WORDS;
    {
        QForm x;
        qf_load(c, x, base + g * base_stride * REC_WORDS);
        qf_store(c, x, tab);
    }
    const int len = (int)*maxlen;
    const uint32_t table_steps = tw > 1 ? tw : 0;       // 1 squaring + tw - 1 products
    uint32_t ts = 0;
    int t = len - 1;
    bool have = false, mul_pending = false;
    // one composition per iteration and ONE qf_compose call site; the schedule is the same for every
    // group (shared exponent), so the branches below are uniform over the workgroup
    while (true) {
        const uint32_t *lsrc = accp, *rsrc = nullptr;     // rsrc == nullptr: a squaring
        uint32_t *dst = accp;
        bool rinv = false;
        if (ts < table_steps) {
            if (ts == 0) {                                // x^2 -> slot tw
                lsrc = tab;
                dst = tab + (uint64_t)tw * REC_WORDS;
            } else {                                      // x^(2 ts + 1) = x^(2 ts - 1) o x^2 -> slot ts
                lsrc = tab + (uint64_t)(ts - 1) * REC_WORDS;
                rsrc = tab + (uint64_t)tw * REC_WORDS;
                dst = tab + (uint64_t)ts * REC_WORDS;
            }
        } else if (t < 0) {
            break;
        } else if (!have) {
            const int dg = digits[t];                     // leading digit: non-zero by construction
            QForm f;
            qf_load(c, f, tab + (uint64_t)((dg < 0 ? -dg : dg) >> 1) * REC_WORDS);
            if (dg < 0) qf_inverse(c, f);
            qf_store(c, f, accp);
            have = true;
            t--;
            continue;
        } else if (!mul_pending) {
            mul_pending = digits[t] != 0;
            if (!mul_pending) t--;
        } else {
            const int dg = digits[t];
            rsrc = tab + (uint64_t)((dg < 0 ? -dg : dg) >> 1) * REC_WORDS;
            rinv = dg < 0;
            mul_pending = false;
            t--;
        }
        QForm l_, r_, r;
        qf_load(c, l_, lsrc);
        if (rsrc) {
            qf_load(c, r_, rsrc);
            if (rinv) qf_inverse(c, r_);
        } else {
            r_ = l_;
        }
        qf_compose<WG, false, false>(c, r, l_, r_, dd);
        qf_store(c, r, dst);
        if (ts < table_steps) ts++;
    }
    if (alive) {
        QForm acc;
        qf_load(c, acc, len == 0 ? one_rec : (const uint32_t *)accp);
        qf_store(c, acc, out + g * REC_WORDS);
    }
}
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_pow_shared(const uint32_t *__restrict__ base, const int8_t *__restrict__ digits,
                                                                    const uint32_t *__restrict__ maxlen, uint32_t *__restrict__ table,
                                                                    uint32_t *__restrict__ out, uint64_t n_items, uint32_t base_stride,
                                                                    uint32_t tw, const uint32_t *__restrict__ one_rec,
                                                                    const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    pow_shared_body<1>(c, base, digits, maxlen, table, out, n_items, base_stride, tw, one_rec, absdelta, half_dbits, status);
}
__global__ void __launch_bounds__(64) k_pow_shared_solo(const uint32_t *__restrict__ base, const int8_t *__restrict__ digits,
                                                        const uint32_t *__restrict__ maxlen, uint32_t *__restrict__ table,
                                                        uint32_t *__restrict__ out, uint64_t n_items, uint32_t base_stride,
                                                        uint32_t tw, const uint32_t *__restrict__ one_rec,
                                                        const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[(64 / G) * SCRATCH_WORDS];
    Ctx c = make_ctx(lds);
    c.rank = -1;
    pow_shared_body<0>(c, base, digits, maxlen, table, out, n_items, base_stride, tw, one_rec, absdelta, half_dbits, status);
}
#endif

// Decryption (reference: CPUCryptoSystem::decrypt_tensor, cpu_cryptosystem_tensor_ops.inl:21-33 ->
// CL_HSM2k::decrypt; threshold form: finalDecrypt / compute_d, cpu_cryptosystem_distributed.inl:231-285).
// Input per ciphertext: d = prod_i parts[i * n_ct + g]^(+-1) (bit i of negmask = exponent -1) -- the
// parties' partial decryptions c1^share_i, or the single c1^sk of ordinary decryption (k_pow_shared).
// c2 o d^-1 is an element f^m of the cyclic subgroup F of order 2^k, and its exponent is read off bit
// by bit from the bottom: the reduced form of f^m has first coefficient 2^(2(k-j)) with j the 2-adic
// valuation of m, so multiplying by the tabulated f^(-2^j) clears the lowest set bit of m and exposes
// the next one (at most k, on average k/2 compositions).  ftab[2j] = f^(-2^j).
// Output per ciphertext: ceil(k/32) words of m, then one status word (0 = ok, 1 = not in <f>).
#if PART_HAS(2)
__device__ __forceinline__ void k_decrypt_body(const uint32_t *__restrict__ cts, const uint32_t *__restrict__ parts,
                                                                 uint32_t n_parts, uint64_t negmask,
                                                                 const uint32_t *__restrict__ ftab, uint32_t *__restrict__ out,
                                                                 uint64_t n_ct, int kbits, const uint32_t *__restrict__ absdelta,
                                                                 int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_LDS_WORDS];
    Ctx c = make_wg_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < n_ct;
    const uint64_t g = alive ? g0 : n_ct - 1;
    const int mwords = (kbits + 31) / 32;
    uint32_t *o = out + g * (uint64_t)(mwords + 1);
    if (alive)
        for (int i = c.gl; i <= mwords; i += G) o[i] = 0;
    QForm acc;
    const uint32_t *dummy = parts + g * REC_WORDS;
    qf_load(c, acc, dummy);
    if (negmask & 1) qf_inverse(c, acc);
    uint32_t pj = 1;                  // next partial decryption to fold in
    int stage = 0;                    // 0: product of the parts, 1: c2 o acc^-1, 2: peel m, 3: done
    uint32_t mw = 0, verdict = 0;     // current word of m; 1 = not an element of <f>
    int mwi = 0, steps = 0;
    while (true) {
        QForm lhs = acc, rhs;
        bool has = false;
        while (alive && stage < 3 && !has) {
            if (stage == 0) {
                if (pj >= n_parts) {
                    stage = 1;
                    continue;
                }
                qf_load(c, rhs, parts + ((uint64_t)pj * n_ct + g) * REC_WORDS);
                if ((negmask >> pj) & 1) qf_inverse(c, rhs);
                pj++;
                has = true;
            } else if (stage == 1) {
                qf_inverse(c, lhs);                                  // d^-1
                qf_load(c, rhs, cts + (2 * g + 1) * REC_WORDS);
                stage = 2;
                has = true;
            } else {
                if (mp_is_word(c, acc.a, 1)) {                       // identity: every bit of m is out
                    stage = 3;
                    continue;
                }
                const int e = mp_bitlen(c, acc.a) - 1;
                const int j = kbits - e / 2;
                if ((e & 1) || j < 0 || j >= kbits || steps > kbits || (j >> 5) < mwi) {
                    verdict = 1;                                     // not an element of <f>
                    stage = 3;
                    continue;
                }
                steps++;
                if ((j >> 5) != mwi) {
                    if (c.gl == 0) o[mwi] = mw;
                    mw = 0;
                    mwi = j >> 5;
                }
                mw |= 1u << (j & 31);
                qf_load(c, rhs, ftab + (uint64_t)(2 * j) * REC_WORDS);
                has = true;
            }
        }
        if (!__syncthreads_or(has ? 1 : 0)) break;
        QForm r;
        WG_ROUND(has, lhs, rhs, dummy, r);
        // unconditionally: a group without a composition of its own has finished (stage 3) or lies beyond the tensor and never
        // reads its running product again -- keeping the old value "if (!has)" made the form live across the whole of
        // qf_compose (20 registers spilled and reloaded around ~55 k instructions for nothing)
        acc = r;
    }
    if (alive && c.gl == 0) {
        o[mwi] = mw;
        o[mwords] = verdict;
    }
}
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_decrypt(const uint32_t *__restrict__ cts, const uint32_t *__restrict__ parts,
                                                                 uint32_t n_parts, uint64_t negmask,
                                                                 const uint32_t *__restrict__ ftab, uint32_t *__restrict__ out,
                                                                 uint64_t n_ct, int kbits, const uint32_t *__restrict__ absdelta,
                                                                 int half_dbits, uint32_t *__restrict__ status) {
    k_decrypt_body(cts, parts, n_parts, negmask, ftab, out, n_ct, kbits, absdelta, half_dbits, status);
}
// three workgroups per CU (see k_compose_wg3): for grids of at most 768 workgroups
__global__ void __launch_bounds__(WG_BLOCK, 3) k_decrypt3(const uint32_t *__restrict__ cts, const uint32_t *__restrict__ parts,
                                                                 uint32_t n_parts, uint64_t negmask,
                                                                 const uint32_t *__restrict__ ftab, uint32_t *__restrict__ out,
                                                                 uint64_t n_ct, int kbits, const uint32_t *__restrict__ absdelta,
                                                                 int half_dbits, uint32_t *__restrict__ status) {
    k_decrypt_body(cts, parts, n_parts, negmask, ftab, out, n_ct, kbits, absdelta, half_dbits, status);
}
#endif

// (Encryption with given randomness -- reference encrypt_tensor, cpu_cryptosystem_tensor_ops.inl:1-19 -- has no chain kernel
// any more: f^(m_i) o pk^r is a product of table entries, multiplied out by k_encrypt_select + k_gather_signed + the
// k_compose_pairs tree in cofhe_hip_encrypt_records.)

}  // namespace cofhe_k
