// Host build of the per-thread bodies of k_unpack, k_widths and k_pack (cofhe_amd/csrc/wire.hpp): the very functions the
// kernels call, driven by plain loops over the thread index in the kernels' own order and over the kernels' own grids (whole
// blocks of 256, so the threads past the end run too).  The exclusive prefix sum that k_tile_sums, k_scan_tiles and k_offsets
// compute between k_widths and k_pack is a SERIAL sum here: the scan kernels are not simulated (tests/test_gpu_wire.py runs
// them).  Every output buffer is filled with 0xA5 before a body runs, so a byte that was never written is seen.
// TEST INFRASTRUCTURE ONLY; not linked into the product library.
#define COFHE_HOSTSIM 1
#include <string.h>

#include <vector>

#include "../../cofhe_amd/csrc/wire.hpp"

using namespace cofhe;

namespace {
uint64_t grid_threads(uint64_t threads) { return (threads + 255) / 256 * 256; }
}  // namespace

extern "C" {
int wire_sim_rec_words(int kind) { return geometry(kind).rec_words; }
int wire_sim_ints_per_rec(int kind) { return geometry(kind).ints_per_rec; }
int wire_sim_pack_groups(int kind) { return wire_pack_groups(kind); }

// k_unpack over n_rec records: rec has rec_cap_words words, all 0xA5A5A5A5 before the first thread; returns the err word
uint32_t wire_sim_unpack(const uint8_t *body, const uint64_t *off, uint64_t body_len, uint64_t n_rec, int kind, uint32_t *rec,
                         uint64_t rec_cap_words) {
    memset(rec, 0xA5, rec_cap_words * 4);
    uint32_t err = 0;
    const uint64_t threads = grid_threads(n_rec * geometry(kind).rec_words);
    for (uint64_t tid = 0; tid < threads; tid++) {
        const UnpackWord u = wire_unpack_word(body, off, body_len, n_rec, kind, tid);
        err |= u.err;
        if (u.store) {
            if (tid >= rec_cap_words) return 0x80000000u;      // a store outside the buffer: not made, reported
            rec[tid] = u.val;
        }
    }
    return err;
}

// k_widths, the prefix sum, k_pack: off[count] and body[body_cap] are 0xA5 before the first thread; *body_len = the sum of
// the widths.  Returns 0, or -1 when the body does not fit (nothing packed then, as in cofhe_hip_pack_tensor_device).
int wire_sim_pack(const uint32_t *rec, uint64_t n_rec, int kind, uint64_t *off, uint8_t *body, uint64_t body_cap, uint64_t *body_len) {
    const uint64_t count = n_rec * geometry(kind).ints_per_rec;
    memset(off, 0xA5, count * 8);
    memset(body, 0xA5, body_cap);
    std::vector<uint64_t> width(count);
    for (uint64_t j = 0; j < grid_threads(count); j++)
        if (j < count) width[j] = wire_width(rec, kind, j);          // k_widths' own guard
    uint64_t run = 0;
    for (uint64_t j = 0; j < count; j++) {
        off[j] = run | (width[j] & ~WIRE_OFFMASK);
        run += width[j] & WIRE_OFFMASK;
    }
    *body_len = run;
    if (run > body_cap) return -1;
    const int max_words = wire_pack_groups(kind);
    for (uint64_t tid = 0; tid < grid_threads(count * (uint64_t)max_words); tid++)
        wire_pack_group(rec, off, width.data(), n_rec, kind, max_words, body, tid);
    return 0;
}
}
