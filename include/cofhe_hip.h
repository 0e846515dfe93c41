/* cofhe_hip.h -- C ABI of the MI355X evaluation engine for CoFHE's local ciphertext-tensor
 * path.  Plain pointers and sizes only; no C++, GMP or torch types cross this boundary.
 *
 * What each entry point replaces in the reference (paths under /root/reference):
 *   cofhe_hip_compose_records        the hot loop of CPUCryptoSystem::add_ciphertext_tensors,
 *                                    include/x86_64/cpu_cryptosystem_tensor_ops.inl:242-264
 *                                    (Cl_G.nucomp / Cl_Delta.nucomp per element)
 *   cofhe_hip_pow_records            the 1-D branch of scal_ciphertext_tensors,
 *                                    cpu_cryptosystem_tensor_ops.inl:316-338 (ClassGroup::nupow)
 *                                    and negate_ciphertext_tensor, :170-192
 *   cofhe_hip_scal_matmul_records    the 2-D branch, cpu_cryptosystem_tensor_ops.inl:342-461
 *                                    (qfi_nupow tables, include/x86_64/qfi.inl:1-135, fused
 *                                    with the accumulation loop :403-417)
 *   cofhe_hip_matmul_plain_ct_...    nothing: the plaintext matrix on the LEFT of the ciphertext matrix (y = W x); the
 *                                    reference's 2-D branch is ciphertext-left only
 *   cofhe_hip_matmul_plain_plain_... nothing: a plaintext matrix product mod 2^k, the E D term of a matrix Beaver
 *                                    triplet (include/smpc/ciphertext_multiplications.hpp:51-111 expands into elements)
 *   cofhe_hip_conv2d_plain_ct_...    nothing: the reference has no convolution; with it, plaintext filters over an encrypted image
 *                                    are a patch matrix built by the caller and the 2-D branch above
 *   cofhe_hip_conv2d_grouped_...,    nothing: the same with dilation and groups (depthwise filters, per-channel scales), and sum
 *   cofhe_hip_sum_pool2d_...         pooling as the depthwise convolution with filters of ones
 *   cofhe_hip_conv2d_ct_filters_..., nothing: ciphertext filters over an opened image and the plaintext convolution mod 2^k, the
 *   cofhe_hip_conv2d_plain_plain_... E * [Bf] and E * D terms of a convolution Beaver triplet
 *   cofhe_hip_pow_dot_records,       nothing: a polynomial with plaintext coefficients on a ciphertext tensor from ONE opened
 *   cofhe_hip_poly_shift_records,    value per element (power tuples); ComputeOperation's POLYNOMIAL_EVALUATION is commented out
 *   cofhe_hip_poly_close_...         (include/node/compute_request_handler.hpp:74)
 *   cofhe_hip_divfloor_plain_...,    nothing: a ciphertext tensor divided by public divisors (rescale, mean, average pool) from ONE
 *   cofhe_hip_div_close_...          opened value per element (division pairs); ComputeOperation::DIVIDE answers "Not implemented"
 *                                    (include/node/compute_request_handler.hpp:73, 343-344)
 *   cofhe_hip_lut_rotate_...,        nothing: ANY public function of a b-bit value on a ciphertext tensor, exactly (ReLU, max, max
 *   cofhe_hip_lut_tuples_...,        pooling), from ONE opened value per element (lookup tuples); the reference has no comparison
 *   cofhe_hip_lut_select_...         and no table lookup
 *   cofhe_hip_spline_rows_...,       nothing: a piecewise polynomial (sigmoid, tanh, GELU, exp, 1/x as splines) over a (shift + bits)-bit
 *   cofhe_hip_spline_tuples_...,     window on a ciphertext tensor from ONE opened value per element (spline tuples of 2^bits (d + 1)
 *   cofhe_hip_spline_close_...       ciphertexts, not 2^(shift + bits)); the reference has no such operation
 *   cofhe_hip_cmp_rows_...,          nothing: the exact sign (ReLU, max) of a value on a window of up to 64 bits, from digit
 *   cofhe_hip_cmp_tuples_...,        comparisons against a masked opened value and one small lookup (comparison tuples of
 *   cofhe_hip_cmp_close_...          ceil(bits / d) 2^d ciphertexts, not 2^bits); the reference has no comparison
 *   cofhe_hip_decrypt_records        decrypt_tensor's per-element work, cpu_cryptosystem_tensor_ops.inl:21-33
 *   cofhe_hip_part_decrypt_records,  part_decrypt_tensor / combine_part_decryption_results_tensor,
 *   cofhe_hip_combine_part_...       cpu_cryptosystem_tensor_ops.inl:35-73 (cpu_cryptosystem_distributed.inl:231-285)
 *   cofhe_hip_*_bytes                the same three operations on the reference's binary tensor
 *                                    format (serialize/deserialize_ciphertext_tensor,
 *                                    include/x86_64/cpu_cryptosystem.inl:320-508; plaintext
 *                                    tensors :229-318), i.e. what a Tensor<CipherText*> call
 *                                    site hands over after serialising
 *   cofhe_hip_bytes_to_records /     the (de)serialisers themselves, producing / consuming the
 *   cofhe_hip_records_to_bytes       device layout (cofhe_amd/csrc/layout.hpp)
 *
 * Records: one quadratic form = 168 little-endian u32 words (a[40] |b|[40] c[80] sign pad[7]);
 * one ciphertext = 2 records (c1, c2).  Exponents: EXP_WORDS u32 magnitude words + 1 sign
 * word each (cofhe_hip_exp_words()).
 *
 * Concurrency: a context may be shared by host threads: the entry points that use its grow-only workspace, its
 * cached tables or its status area (matrix product, encrypt, decrypt, part_decrypt, combine, accumulate, validate,
 * device_status, the *_bytes operations) take the context's lock for the duration of the call; their kernels run
 * in stream order.  Calls on DIFFERENT streams of one context (cofhe_hip_stream_create) are safe, not concurrent: the last
 * user of the workspace records an event and the next one's stream waits for it, tables are built before their readers
 * run, and a block of the block cache is handed out again only after the work queued behind its free.  What a caller
 * orders itself is its own data: a buffer written on one stream and read on another.  compose / pow / the converters are
 * stateless.
 *
 * All functions return 0 on success, a negative COFHE_HIP_E* code otherwise;
 * cofhe_hip_last_error() gives the message for the calling thread.  The library never falls
 * back to a CPU computation: without a usable GPU cofhe_hip_ctx_create fails.
 */
#ifndef COFHE_HIP_H
#define COFHE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COFHE_HIP_OK 0
#define COFHE_HIP_EINVAL (-1)   /* malformed buffer / value exceeds the limb capacity        */
#define COFHE_HIP_ESHAPE (-2)   /* "Tensor shapes must be equal" / "Vector sizes must be equal" */
#define COFHE_HIP_ENDIM (-3)    /* "Tensors must be 0D, 1D or 2D for now"                      */
#define COFHE_HIP_EHIP (-4)     /* HIP runtime error (message carries hipGetErrorString)       */
#define COFHE_HIP_ENOMEM (-5)

typedef struct cofhe_hip_ctx cofhe_hip_ctx;

const char *cofhe_hip_last_error(void);
int cofhe_hip_record_words(void);   /* 168 */
int cofhe_hip_exp_words(void);      /* magnitude words per exponent (sign word follows) */

/* Context bound to one GPU and one discriminant; absdelta = little-endian bytes of |Delta|. */
int cofhe_hip_ctx_create(int device, const uint8_t *absdelta_le, size_t len, cofhe_hip_ctx **out);
void cofhe_hip_ctx_destroy(cofhe_hip_ctx *ctx);

/* device memory (so a host language needs no HIP binding).  Freed blocks are kept by the context and handed out again
 * for the same size class (at most 12.5 % above the request): cofhe_hip_free does not synchronise the device as hipFree does -- the block is
 * reused only after everything that was submitted to the null stream or a blocking stream before the free has run.
 * Buffers last used on a NON-blocking stream (PyTorch's pool streams are) are freed with cofhe_hip_free_on_stream,
 * which orders the reuse after the work queued on that stream.  When the device runs out of memory (here, for the
 * context's workspace or its tables) the cache is released and the allocation retried.
 * cofhe_hip_trim(ctx, keep) sets the cache limit (default: an eighth of the device memory, at most 64 GiB) and
 * releases the cache if it holds more. */
int cofhe_hip_malloc(cofhe_hip_ctx *ctx, size_t bytes, void **dptr);
int cofhe_hip_free(cofhe_hip_ctx *ctx, void *dptr);
int cofhe_hip_free_on_stream(cofhe_hip_ctx *ctx, void *dptr, void *stream);
int cofhe_hip_trim(cofhe_hip_ctx *ctx, size_t keep_bytes);
/* Launcher decisions of the matrix product that a caller may pin (0 = automatic, the default):
 *   "wnaf_width"       2..8: window width of the exponent recoding (automatic: minimises table + chain work)
 *   "ladder_form"      shared-exponent ladders (decryption): 0 by their number, 1 a pair of wavefronts per ladder (wide
 *                      layout: one squares, one multiplies), 2 the 8-lane in-wave form (<= 8 ladders), 3 the throughput
 *                      kernel, 4 one wavefront per ladder (wide layout, left to right with a table)
 *   "matmul_tree"      -1: the launcher decides; 1: the matrix product as per-position product trees + a Horner chain
 *                      wherever its encoding allows (at most 2^21 non-empty (bit position, column) segments; beyond that the
 *                      chains run); 0: lockstep chains (the form of rounds 1-3)
 *   "matmul_segments"  >= 1: pieces the inner dimension is cut into when the product has few outputs
 *   "comb_width"       2..10: window width of the fixed-base comb (cofhe_hip_pow_fixed_base_many_records and kin)
 *   "comb_chunk"       >= 1: items per pass of the comb (capped where the 4 GiB workspace bound needs it)
 *   "conv_route"       cofhe_hip_conv2d_plain_ct_records, cofhe_hip_conv2d_grouped_plain_ct_records and
 *                      cofhe_hip_sum_pool2d_records: 0 the launcher decides, 1 the direct route wherever it does not decline, 2 the
 *                      gather route (with groups: wherever its dense patch matrix fits)
 *   "conv_chunk_rows"  >= 1: output positions per chunk of the convolution's direct route, taken as given (no rounding to a
 *                      multiple of 16, no decline for being small): how a test reaches several chunks and workgroups that
 *                      mix tree elements
 *   "view_grid_blocks" >= 1: the grid of cofhe_hip_view_records and cofhe_hip_gather_records, taken as given: how a test reaches
 *                      their grid-stride loops with a thousand records
 *   "profile_kernels"  != 0: cofhe_hip_scal_matmul_records brackets each of its kernels with HIP events on the launch
 *                      stream; cofhe_hip_profile_read(ctx, "k_tree_level" | "k_scal_matmul_wnaf" | "k_pow_table" | "k_wnaf_digits", ...)
 *                      waits for them and returns the summed duration and the launch count (clear != 0 drops all spans).
 *                      The three-per-CU builds get a span of their own inside those ("k_scal_matmul_wnaf3", "k_pow_table3"),
 *                      and the kernels of the other entry points one named after the build launched: "k_compose_wg3" |
 *                      "k_compose_wg", "k_add_ct3" | "k_add_ct", "k_pow_shared_pair" | "k_pow_shared_wide" |
 *                      "k_pow_shared_solo" | "k_pow_shared" (ladders; "k_spread_records" when a
 *                      tensor's shared c1 ran one ladder), "k_decrypt3" | "k_decrypt", "k_conv_level0" (one per chunk of the
 *                      convolution's direct route; "k_tree_level" counts the levels above) | "k_gather_patches" (its
 *                      gather route, after "k_expand_group_filters" when the convolution has groups) -- what a test reads to see
 *                      which route a call took
 * The results do not depend on them; tests pin them to drive every width through the parity checker. */
int cofhe_hip_ctx_set_option(cofhe_hip_ctx *ctx, const char *name, int64_t value);
int cofhe_hip_profile_read(cofhe_hip_ctx *ctx, const char *kernel, float *total_ms, uint32_t *launches, int clear);
int cofhe_hip_upload(cofhe_hip_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes, void *stream);
int cofhe_hip_download(cofhe_hip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes, void *stream);
int cofhe_hip_stream_sync(cofhe_hip_ctx *ctx, void *stream);
/* Streams of the library's own HIP runtime, on the context's device: what a client that serves several worker threads from one
 * context gives each of them.  (A process that also holds PyTorch holds two HIP runtimes; a torch.cuda.Stream handle belongs to
 * the other one and means nothing here.)  nonblocking != 0: hipStreamNonBlocking -- the null stream neither waits for such a
 * stream nor is waited for by it; 0: a blocking stream.  cofhe_hip_stream_destroy waits for the work queued on the stream, then
 * releases it; the context forgets it as the last user of its workspace, so that a later stream with the same handle value
 * is not taken for it, and lets go of every event it recorded on it (the blocks of the block cache that were freed behind
 * it: a HIP event names the stream it was last recorded on, and waiting for one whose stream is gone fails).  So a stream that
 * was handed to this library is ended HERE, not with hipStreamDestroy, and "profile_kernels" spans recorded on it are read
 * (cofhe_hip_profile_read) before it goes.  A null stream is a no-op.  cofhe_hip_stream_query: *busy = 1 while work queued on
 * the stream is pending (hipStreamQuery), 0 when it is idle; it does not wait.  COFHE_HIP_EINVAL for a null ctx or out-pointer. */
int cofhe_hip_stream_create(cofhe_hip_ctx *ctx, int nonblocking, void **stream);
int cofhe_hip_stream_destroy(cofhe_hip_ctx *ctx, void *stream);
int cofhe_hip_stream_query(cofhe_hip_ctx *ctx, void *stream, int *busy);

/* Device status word: every data-dependent loop of the kernels has a trip-count cap; a cap that is hit (possible only
 * for records that are not reduced forms of the context's discriminant) sets a bit instead of hanging or passing
 * silently: 1 = remainder sequence, 2 = reduction, 4 = division (by zero / no end).  32 = cofhe_hip_gather_records met
 * an index beyond its source (nothing was read there).  clear != 0 resets it.
 * Synchronises `stream`. */
int cofhe_hip_device_status(cofhe_hip_ctx *ctx, uint32_t *word, int clear, void *stream);
/* *all_valid = 1 when every one of the n form records is a reduced, primitive form of the context's discriminant
 * (a, c > 0, |b| <= a <= c, canonical sign, b^2 - 4ac = Delta, and a, b, c not all even: for a CL_HSM2k discriminant
 * that is gcd(a, b, c) = 1, for one with an odd square factor it is necessary only).  cofhe_hip_unpack_tensor_device and the *_bytes
 * operations run this on everything they deserialise; records produced by the kernels themselves need no check.
 * Synchronises `stream`. */
int cofhe_hip_validate_records(cofhe_hip_ctx *ctx, const void *d_records, uint64_t n_records, int *all_valid, void *stream);

/* ---- kernels on device-resident records (stream: hipStream_t, NULL = default stream) ---- */
/* out[i] = a[i] o b[i] for n_records forms (a ciphertext tensor of E elements is 2E records) */
int cofhe_hip_compose_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out,
                              uint64_t n_records, void *stream);
/* out[i] = a[i] o b[i], ONE composition per wavefront in the wavefront-wide layout (csrc/wide.hpp: two limbs per lane over the
 * 64 lanes, no workgroup protocol): the composition of the latency kernels -- the ladders of cofhe_hip_decrypt_records /
 * cofhe_hip_part_decrypt_records when there are few of them -- as an entry of its own, for parity tests and for timing one
 * composition by itself (reps > 1 repeats it inside the kernel).  Same result records as cofhe_hip_compose_records.
 * *fallbacks (optional): how many pairs the wide route declined and took through the 8-lane code (synchronises). */
int cofhe_hip_compose_wide_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n_records,
                                   uint32_t reps, uint32_t *fallbacks, void *stream);
/* out[i] = a[i] + b[i] for n_ct ciphertexts (2 records each; same result records as cofhe_hip_compose_records over
 * 2 n_ct records).  When every ciphertext of a shares one c1 and every ciphertext of b shares one c1 -- tensors that
 * encrypt_tensor made with its one r per tensor (cpu_cryptosystem_tensor_ops.inl:7-12), and sums of such tensors --
 * the composition c1 o c1' is computed once and copied: n_ct + 1 compositions instead of 2 n_ct.  Detected on the
 * device per call (one pass over the c1 records); tensors with differing c1 take the plain path.  d_out may be d_a.
 * The verdict of that pass lives in one of the context's 256 flag words, handed out round robin: purely stream-ordered, no
 * read-back, and safe on any number of streams as long as at most 256 flag-using calls of one context are in flight (queued
 * and not yet run) at a time; the 257th would reuse the word of the first. */
int cofhe_hip_add_ciphertext_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n_ct, void *stream);
/* out[i] = a[i] - b[i]: (a.c1 o b.c1^-1, a.c2 o b.c2^-1), one composition per record -- the inverse of a reduced form is a
 * sign flip -- where negate (b^(2^k - 1), k squarings and a product per record) followed by an addition spends k + 2.  Folding
 * of a shared c1 and launch routes as cofhe_hip_add_ciphertext_records; d_out may be d_a or d_b.  "profile_kernels" spans
 * "k_sub_ct3" | "k_sub_ct".  Reference: the compute node's SUBTRACT, which answers "Not implemented"
 * (include/node/compute_request_handler.hpp:67-76, 342-344). */
int cofhe_hip_sub_ciphertext_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint64_t n_ct, void *stream);
/* out[i] = in[i]^-1 on form records (a ciphertext tensor: 2 n_ct records): Enc(-m) at no composition, a ciphertext other
 * than negate_ciphertext_tensor's ct^(2^k - 1) (tensor_ops.inl:431-460) with the same plaintext; in place allowed. */
int cofhe_hip_invert_records(cofhe_hip_ctx *ctx, const void *d_in, void *d_out, uint64_t n_records, void *stream);
/* out[2e+h] = base[2e+h] ^ exp[e] for E ciphertexts (h = 0,1) */
int cofhe_hip_pow_records(cofhe_hip_ctx *ctx, const void *d_base, const void *d_exp, void *d_out,
                          uint64_t n_ciphertexts, void *stream);
/* out[i,k] = zero o prod_j cts[i,j]^s[j,k];  cts n x m, s m x p (exponent records), zero 1 ct.
 * NOT purely stream-ordered: the call synchronises `stream` once or twice before it returns its last launches -- the
 * window width follows the longest exponent (a 4-byte read-back) and the product tree is sized by per-level totals (a
 * ~100-byte read-back); the launches that follow are asynchronous as everywhere else. */
int cofhe_hip_scal_matmul_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_exp,
                                  const void *d_zero, void *d_out, uint32_t n, uint32_t m, uint32_t p,
                                  void *stream);
/* The plaintext-LEFT product: out[i,k] = zero o prod_j cts[j,k]^s[i,j];  s n x m (exponent records), cts m x p, out n x p,
 * zero 1 ct -- a linear layer y = W x with plaintext weights and encrypted activations.  The reference has no such
 * operation (its 2-D scal_ciphertext_tensors has the ciphertext matrix on the left).  Runs cofhe_hip_scal_matmul_records on
 * transposed views, out^T (p x n) = cts^T (p x m) . s^T (m x n): three transposes of fixed-size records around the existing
 * routes, which keep their width choice, tree / chains / segments and options.  The class group is commutative and the
 * reduced form unique, so the bytes are those of any other order of the factors.  The three temporaries (2 m p and 2 n p
 * form records, n m exponent records) come from the context's block cache and go back behind the work queued on `stream`.
 * Inherited from cofhe_hip_scal_matmul_records: m < 2^21, 2 n p records within the launch limit, and its one or two
 * synchronisations of `stream` (NOT purely stream-ordered).  d_out must not overlap d_s, d_cts or d_zero: COFHE_HIP_EINVAL,
 * nothing written.  n p == 0: nothing to do; m == 0: zero everywhere. */
int cofhe_hip_matmul_plain_ct_records(cofhe_hip_ctx *ctx, const void *d_s, const void *d_cts, const void *d_zero, void *d_out,
                                      uint32_t n, uint32_t m, uint32_t p, void *stream);
/* 2-D convolution of a ciphertext image with plaintext filters, channels last (cofhe_amd/csrc/conv.hpp):
 *   image d_cts [B, H, W, C] ciphertexts, filters d_w [kh, kw, C, Co] exponent records, output d_out [B, Ho, Wo, Co],
 *   out[b,oy,ox,co] = zero o prod_{dy,dx,ci} cts[b, oy sh + dy - ph, ox sw + dx - pw, ci] ^ w[dy,dx,ci,co],
 * factors outside the image left out (zero padding), Ho = (H + 2 ph - kh) / sh + 1 and Wo likewise, rounded down.  Read as
 * matrices the filters are the m x p exponent matrix of cofhe_hip_scal_matmul_records (m = kh kw C, p = Co) and the output its
 * n x p result (n = B Ho Wo), so a layer's output is the next layer's input and nothing is rearranged.  The reference has no
 * convolution.  Two routes ("conv_route"): the direct one builds the table of odd powers ONCE over the image and lets level 0 of
 * the product tree find its leaves in it -- no patch matrix (im2col), whose kh kw copies of every ciphertext would each get a
 * table of their own; the gather route writes the patch matrix into a block of the block cache and runs
 * cofhe_hip_scal_matmul_records on it unchanged, when the direct route declines (as the matrix product's tree does) or for small
 * shapes.  The window width follows the matrix product's cost model with a pixel's table amortised over the
 * ceil(kh/sh) ceil(kw/sw) windows it is in; "wnaf_width" pins it.  Zero weights cost nothing, so sum pooling or a strided
 * subsampling written as a 0/1 filter run at their real cost.
 * COFHE_HIP_EINVAL, nothing written: a stride of 0; ph >= kh or pw >= kw; kh > H + 2 ph or kw > W + 2 pw; m >= 2^21; B H W C
 * above 2^31 - 1, n above 2^32 - 1, n m above 2^40 or 2 n p records beyond the launch limit; d_out overlapping d_w, d_cts or
 * d_zero.  B Ho Wo Co == 0: nothing to do.  NOT purely stream-ordered: as cofhe_hip_scal_matmul_records, the call synchronises
 * `stream` once or twice.  Dilation and groups / depthwise filters: cofhe_hip_conv2d_grouped_plain_ct_records below;
 * ciphertext filters: cofhe_hip_conv2d_ct_filters_records.  Not covered: a per-channel bias, which is
 * cofhe_hip_add_plain_records on the result. */
typedef struct {
    uint32_t B, H, W, C;       /* image */
    uint32_t kh, kw, Co;       /* filters: kh x kw x C x Co */
    uint32_t sh, sw, ph, pw;   /* strides, zero padding (rows, columns) */
} cofhe_hip_conv2d_shape;
/* host only, no GPU: validates the shape (COFHE_HIP_EINVAL for the refusals above) and gives the output extents */
int cofhe_hip_conv2d_out_shape(const cofhe_hip_conv2d_shape *shape, uint32_t *Ho, uint32_t *Wo);
int cofhe_hip_conv2d_plain_ct_records(cofhe_hip_ctx *ctx, const void *d_w, const void *d_cts, const void *d_zero, void *d_out,
                                      const cofhe_hip_conv2d_shape *shape, void *stream);
/* The same convolution with dilation and groups:
 *   filters d_w [kh, kw, C / groups, Co];  with Cg = C / groups, Cog = Co / groups,
 *   out[b,oy,ox,co] = zero o prod_{dy,dx,ci<Cg} cts[b, oy sh + dy dh - ph, ox sw + dx dw - pw, (co / Cog) Cg + ci] ^ w[dy,dx,ci,co],
 * Ho = (H + 2 ph - ((kh - 1) dh + 1)) / sh + 1 and Wo likewise.  groups = C = Co is a depthwise convolution; kh = kw = 1 on top of
 * that a per-channel scale (a folded batch norm).  dh = dw = groups = 1 is cofhe_hip_conv2d_plain_ct_records, launch for launch.
 * The matrix view has m = kh kw C / groups: the digits, the segment scans, the filter upload and the 2^21 limit are those of the
 * grouped filter, not of the block-diagonal dense one.  The direct route reads each leaf from the channel block of its column's
 * group (a segment of the product tree belongs to one column).  The gather route expands the filters to the dense
 * [kh, kw, C, Co] tensor in a block of the block cache ("k_expand_group_filters") and runs unchanged; it needs kh kw C < 2^21 and
 * n kh kw C <= 2^40 -- where that does not hold the direct route is forced, and if the direct route then declines the call
 * returns COFHE_HIP_EINVAL and says so.  With groups > 1 the automatic choice is the direct route wherever it does not decline.
 * Further COFHE_HIP_EINVAL, nothing written, checked before the context or a pointer is looked at: a dilation of 0; groups of 0;
 * C or Co not a multiple of groups; with keff = (k - 1) d + 1 in place of k in the refusals above: padding not smaller than keff,
 * keff beyond the padded extent.  A dilated window may lie wholly in the padding: legal, and its outputs are zero.  The overlap
 * check of d_out uses the grouped filter size. */
typedef struct {
    uint32_t B, H, W, C;       /* image */
    uint32_t kh, kw, Co;       /* filters: kh x kw x C / groups x Co */
    uint32_t sh, sw, ph, pw;   /* strides, zero padding (rows, columns) */
    uint32_t dh, dw, groups;   /* dilation (rows, columns), groups */
} cofhe_hip_conv2d_geometry;
/* host only, no GPU: validates the geometry (COFHE_HIP_EINVAL for every refusal) and gives the output extents */
int cofhe_hip_conv2d_geometry_out_shape(const cofhe_hip_conv2d_geometry *geometry, uint32_t *Ho, uint32_t *Wo);
int cofhe_hip_conv2d_grouped_plain_ct_records(cofhe_hip_ctx *ctx, const void *d_w, const void *d_cts, const void *d_zero, void *d_out,
                                              const cofhe_hip_conv2d_geometry *geometry, void *stream);
/* Sum pooling: out[b,oy,ox,c] = zero o prod_{dy,dx} cts[b, oy sh + dy dh - ph, ox sw + dx dw - pw, c], the depthwise convolution
 * with [kh, kw, 1, C] filters of ones, which are made on the device in a block of the block cache.  geometry->Co and
 * geometry->groups are ignored and taken as C.  Exponents of one bit build no table, so an output costs kh kw - 1 compositions
 * per record and the one with zero.  Average pooling is this with the scale 1 / (kh kw) folded into the next layer's plaintext
 * weights: the inverse of kh kw does not exist mod 2^k for an even window.  Refusals, routes and synchronisation as
 * cofhe_hip_conv2d_grouped_plain_ct_records. */
int cofhe_hip_sum_pool2d_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_zero, void *d_out,
                                 const cofhe_hip_conv2d_geometry *geometry, void *stream);
/* out[i,k] = sum_j a[i,j] b[j,k] mod 2^kbits on exponent records (a n x m, b m x p, out n x p; 32 words each: 31 of
 * magnitude and a sign word).  Negative inputs count as -mag mod 2^k and magnitudes of 2^k and above are reduced first; the
 * outputs lie in [0, 2^k) with sign word 0.  1 <= kbits <= 639 (the bound of the decryption table), any kbits in that range:
 * the top limb is masked.  One launch, purely stream-ordered: no workspace, no read-back.  d_out must not overlap the
 * inputs.  The E D term of a matrix Beaver triplet, and the C = A B of its generation. */
int cofhe_hip_matmul_plain_plain_records(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out, uint32_t n, uint32_t m,
                                         uint32_t p, uint32_t kbits, void *stream);
/* ---- convolution with CIPHERTEXT filters from one convolution Beaver triplet (cofhe_amd/csrc/plain_conv.hpp) ----
 * Convolution is bilinear, so the matrix-triplet identity carries over: with a triplet [A] (image-shaped), [Bf] (filter-shaped),
 * [C] = [A * Bf mod 2^k] (output-shaped) and the opened E = Dec(X - A), D = Dec(Wf - Bf),
 *   [X * Wf] = (E * [Bf]) o ([A] * D) o [C] o f^(E * D),
 * which opens B H W C + kh kw C Co values where a matrix triplet on the patch matrix opens n m + m p (every pixel kh kw times) and
 * element triplets 2 n m p.  [A] * D is cofhe_hip_conv2d_grouped_plain_ct_records; the two entry points below are E * D (also the
 * C = A * Bf of the triplet's generation) and E * [Bf].  groups = 1 only: with groups the patch matrix differs per column group.
 * The geometry is cofhe_hip_conv2d_geometry's: channels last, strides, zero padding, dilation.
 *
 * out[b,oy,ox,co] = sum_{dy,dx,ci} img[b, oy sh + dy dh - ph, ox sw + dx dw - pw, ci] w[dy,dx,ci,co] mod 2^kbits on exponent
 * records: image d_img [B, H, W, C], filters d_w [kh, kw, C, Co], output d_out [B, Ho, Wo, Co], terms outside the image left out.
 * An implicit GEMM on the tile of cofhe_hip_matmul_plain_plain_records with the same residue rules (sign word honoured,
 * magnitudes of 2^k and above reduced, outputs in [0, 2^k) with sign word 0, every word of every output record written); no
 * patch matrix is written.  One launch ("k_plain_conv2d"), purely stream-ordered: no workspace, no read-back.
 * COFHE_HIP_EINVAL, nothing written, checked before the context or a pointer is looked at: every refusal of
 * cofhe_hip_conv2d_geometry_out_shape; groups != 1; kbits outside 1..639; d_out overlapping d_img or d_w; Co above 16 * 65535.
 * B Ho Wo Co == 0: nothing to do. */
int cofhe_hip_conv2d_plain_plain_records(cofhe_hip_ctx *ctx, const void *d_img, const void *d_w, void *d_out,
                                         const cofhe_hip_conv2d_geometry *geometry, uint32_t kbits, void *stream);
/* out[b,oy,ox,co] = zero o prod_{dy,dx,ci} filters[dy,dx,ci,co] ^ img[b, oy sh + dy dh - ph, ox sw + dx dw - pw, ci]: a PLAINTEXT
 * image d_img_exps [B, H, W, C] (exponent records) under CIPHERTEXT filters d_filters_cts [kh, kw, C, Co], output d_out
 * [B, Ho, Wo, Co] ciphertexts, zero 1 ct.  Read as matrices this is cofhe_hip_matmul_plain_ct_records with the n x m patch matrix
 * of the image on the left (n = B Ho Wo, m = kh kw C) and the filters as its m x p ciphertext matrix (p = Co).  The patch matrix is
 * written once, already transposed and with the zero exponent in the padding ("k_gather_patch_exponents"), into the block that
 * product would transpose its left operand into -- one pass over n m exponent records less than that call on a pre-gathered
 * patch matrix, and the same bytes.  Everything else is inherited from cofhe_hip_scal_matmul_records on the shape (p, m, n): the
 * routes, the width choice, the options and the one or two synchronisations of `stream` (NOT purely stream-ordered); a
 * filter's table of odd powers is built once and serves all n output positions, and zero exponents cost nothing, so padding is
 * free.  The temporaries (n m exponent records, 2 m p and 2 n p form records) come from the context's block cache and go back
 * behind the work queued on `stream`.  A batch B shares the one filter tensor.
 * COFHE_HIP_EINVAL, nothing written, checked before the context or a pointer is looked at: every refusal of
 * cofhe_hip_conv2d_geometry_out_shape; groups != 1; d_out overlapping d_img_exps, d_filters_cts or d_zero.
 * B Ho Wo Co == 0: nothing to do. */
int cofhe_hip_conv2d_ct_filters_records(cofhe_hip_ctx *ctx, const void *d_img_exps, const void *d_filters_cts, const void *d_zero,
                                        void *d_out, const cofhe_hip_conv2d_geometry *geometry, void *stream);
/* ---- polynomial evaluation from one opened value (cofhe_amd/csrc/pow_dot.hip) ----
 * p(X) = sum_{j<=d} c_j X^j with plaintext coefficients on a ciphertext [x], over the integers mod 2^k.  A POWER TUPLE of an
 * element is ([a], [a^2], .., [a^d]) with a uniform in Z/2^k, used once.  With the ONE opened value e = Dec(x - a), x = a + e and
 *   [p(x)] = (prod_{i=1..d} [a^i]^(q_i(e))) o f^(q_0(e)),   q_i(e) = sum_{j>=i} C(j,i) c_j e^(j-i) mod 2^k   (q_0 = p(e)):
 * one opened value and one round per element whatever d, where d - 1 chained Beaver products open 2 (d - 1) values in d - 1
 * rounds.  The reference has no such operation (ComputeOperation carries a commented-out POLYNOMIAL_EVALUATION,
 * include/node/compute_request_handler.hpp:74).  Fixed-point scales are the caller's: the c_j come pre-scaled so that every
 * term of p carries one scale. */
#define COFHE_HIP_POLY_MAX_DEGREE 8
/* out[2e+h] = prod_{i<d} bases[(i n_ct + e) 2 + h] ^ exps[i n_ct + e], e < n_ct, h in {0, 1}: d ciphertext tensors of n_ct
 * ciphertexts, power-major, each raised element by element to its own exponent tensor (d n_ct exponent records, sign
 * honoured, magnitudes up to 992 bits) and multiplied together -- by ONE ladder per record whose squarings the d bases share:
 * bits + d bits / 3 compositions per record where d calls of cofhe_hip_pow_records and d - 1 additions run d (bits + bits / 3)
 * + d - 1.  Exponents that are all zero give the principal form; d = 1 gives cofhe_hip_pow_records' records.  One launch
 * ("k_pow_dot" under "profile_kernels"), purely stream-ordered: no workspace, no read-back, no lock.  COFHE_HIP_EINVAL, nothing
 * written: d = 0 or d > COFHE_HIP_POLY_MAX_DEGREE; d_out overlapping d_bases or d_exps (the running products live in d_out).
 * n_ct = 0 does nothing. */
int cofhe_hip_pow_dot_records(cofhe_hip_ctx *ctx, const void *d_bases, const void *d_exps, void *d_out, uint64_t n_ct, uint32_t d,
                              void *stream);
/* q[i n + e] = sum_{j>=i} C(j,i) coef[j] x[e]^(j-i) mod 2^kbits, i = 0 .. d: the Taylor shift of the polynomial at every x[e], by
 * repeated synthetic division.  coef: d + 1 exponent records shared by the tensor, x: n, q: (d + 1) n, power-major.  Inputs
 * enter as residues mod 2^kbits and outputs lie in [0, 2^kbits) with sign word 0, as in cofhe_hip_matmul_plain_plain_records;
 * 1 <= kbits <= 639, 0 <= d <= COFHE_HIP_POLY_MAX_DEGREE (d = 0 copies c_0), else COFHE_HIP_EINVAL.  One launch
 * ("k_poly_shift"), purely stream-ordered.  d_q must not overlap the inputs. */
int cofhe_hip_poly_shift_records(cofhe_hip_ctx *ctx, const void *d_coef, const void *d_x, void *d_q, uint64_t n, uint32_t d, uint32_t kbits,
                                 void *stream);
/* The closing step: out[e] = (prod_{i=1..d} powers[i-1][e]^(q_i(e[e]))) o f^(q_0(e[e])), an encryption of p(x[e]) mod 2^kbits when
 * powers[i-1][e] = [a_e^i] and e[e] = x[e] - a_e.  d_coef: d + 1 exponent records; d_e: n_ct; d_powers: d tensors of n_ct
 * ciphertexts, power-major; f_record: HOST record of f.  Three steps on `stream`: cofhe_hip_poly_shift_records into a block
 * of the block cache (which goes back behind the work queued on `stream`), cofhe_hip_pow_dot_records over q_1 .. q_d, and the
 * plaintext addend of cofhe_hip_add_plain_records (mode 0, no randomness) for f^(q_0) against the cached table of f.  Uses
 * the block cache and, through the addend, the workspace plan "comb" (kind 3): it has no plan name of its own.  No read-back.
 * 1 <= d <= COFHE_HIP_POLY_MAX_DEGREE; d_out must not overlap an input (COFHE_HIP_EINVAL). */
int cofhe_hip_poly_close_records(cofhe_hip_ctx *ctx, const void *d_coef, const void *d_e, const void *d_powers, const uint32_t *f_record,
                                 void *d_out, uint64_t n_ct, uint32_t d, uint32_t kbits, void *stream);
/* ---- division by public divisors from one opened value (cofhe_amd/csrc/divide.hip) ----
 * Plaintexts live in Z/2^k; s(v) is the centred residue of v in [-2^(k-1), 2^(k-1)); D is a public divisor, 1 <= D < 2^(k-1).
 * A DIVISION PAIR of an element is ([r], [r_q]) with r uniform in Z/2^k and r_q = floor(s(r) / D) mod 2^k, used once.  With the
 * ONE opened value e = Dec([x] - [r]) -- uniform whatever x is, so it hides x perfectly --
 *   [y] = [r_q] o f^(e_q) = (c1, c2 o f^(e_q)) of [r_q],   e_q = floor(s(e) / D) mod 2^k:
 * no encryption, no ladder.  If s(x) = s(r) + s(e) over the integers, floor(s(x) / D) - s(y) is 0 or 1: the floor quotient or
 * one less.  Otherwise the sum wrapped, which happens with probability |s(x)| / 2^k over r and puts the result off by about
 * 2^k / D.  THE CALLER'S CONTRACT: |x| <= 2^(k-1-sigma) gives a failure probability of at most 2^(-sigma-1) per element (k = 128
 * with 64-bit values: 2^-64).  The reference has no such operation (ComputeOperation::DIVIDE answers "Not implemented",
 * include/node/compute_request_handler.hpp:73, 343-344). */
#define COFHE_HIP_DIV_MAX_KBITS 639
/* q[e] = floor(s(v[e]) / div[e mod n_div]) mod 2^kbits, e < n, on exponent records: the signed floor division, one 8-lane limb
 * group per element.  v enters as a residue mod 2^kbits as in cofhe_hip_matmul_plain_plain_records (sign word honoured,
 * magnitudes of 2^kbits and above reduced, -0 fine) and is negative when bit kbits - 1 of the residue is set; q lies in
 * [0, 2^kbits) with sign word 0.  div: n_div records, element e reads divisor e mod n_div (n_div = 1: a scalar; the channel
 * count of a channels-last tensor: per channel; n: element-wise).  An INVALID divisor (sign word set, residue 0, or 2^(kbits-1)
 * and above) gives quotient 0 and sets the division bit (4) of cofhe_hip_device_status.  One launch ("k_plain_divfloor" under
 * "profile_kernels"), purely stream-ordered: no workspace, no read-back, no lock.  COFHE_HIP_EINVAL, nothing written: kbits = 0 or
 * kbits > COFHE_HIP_DIV_MAX_KBITS; n_div = 0; n no multiple of n_div; d_q overlapping an input.  n = 0 does nothing. */
int cofhe_hip_divfloor_plain_records(cofhe_hip_ctx *ctx, const void *d_v, const void *d_div, uint64_t n_div, void *d_q, uint64_t n,
                                     uint32_t kbits, void *stream);
/* The closing step: out[e] = (c1, c2 o f^(e_q[e])) of rq[e], e_q[e] = floor(s(e[e]) / div[e mod n_div]) mod 2^kbits, an encryption
 * of floor(s(x[e]) / D) or one less when rq[e] = [r_q] of the element's division pair and e[e] = x[e] - r (see above).  d_e: n_ct
 * exponent records; d_div: n_div; d_rq: n_ct ciphertexts; f_record: HOST record of f.  Two steps on `stream`:
 * cofhe_hip_divfloor_plain_records into a block of the block cache (which goes back behind the work queued on `stream`), and the
 * plaintext addend of cofhe_hip_add_plain_records (mode 0, no randomness) on d_rq against the cached table of f.  Uses the block
 * cache and, through the addend, the workspace plan "comb" (kind 3).  No read-back.  d_out must not overlap an input
 * (COFHE_HIP_EINVAL, as for the refusals above). */
int cofhe_hip_div_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_div, uint64_t n_div, const void *d_rq,
                                const uint32_t *f_record, void *d_out, uint64_t n_ct, uint32_t kbits, void *stream);
/* ---- exact floor division and remainders by small public divisors from one opened value (cofhe_amd/csrc/divide_exact.hip) ----
 * The division pair above loses the carry [r mod D + e mod D >= D] of the two remainders: about every second result is one less
 * than the floor.  For a SMALL divisor, 1 <= D <= COFHE_HIP_DIVX_MAX_ROWS and D < 2^(k-1), the party that makes the tuple
 * tabulates that carry over the D remainders the opened value can have.  With q(v) = floor(s(v) / D) and m(v) = s(v) - D q(v) in
 * [0, D), an EXACT-DIVISION TUPLE of an element is ([r], [T_0], .., [T_{D-1}]) with r uniform in Z/2^k and
 * T_j = (q(r) + [m(r) + j >= D]) mod 2^k, used once.  With the ONE opened value e = Dec([x] - [r]) -- uniform whatever x is --
 *   [y] = [T_{m(e)}] o f^(q(e)) = (c1, c2 o f^(q(e))) of [T_{m(e)}]:
 * a copy and a plaintext addend.  If s(x) = s(r) + s(e) over the integers, s(y) = floor(s(x) / D) EXACTLY and the remainder
 * s(x) - D s(y) is (m(r) + m(e)) mod D.  Otherwise the sum wrapped, with the probability and under THE CALLER'S CONTRACT of the
 * division pair: |x| <= 2^(k-1-sigma) for at most 2^(-sigma-1) per element.  EVERY [T_j] MUST CARRY ITS OWN RANDOMNESS, as the
 * entries of a lookup tuple: the rows differ by 0 or 1, so under one shared randomness the quotients of the c2 reveal m(r) and,
 * with e, x mod D; the tuples are made by the fresh-randomness comb (cofhe_hip_divx_tuples_records) and by nothing else.  A tuple
 * of `rows` entries, rows the largest divisor of the call, is rows * 1344 bytes per element: D fresh encryptions against the 2
 * of the inexact pair.  In all entry points element e reads divisor e mod n_div, and an INVALID divisor is one that
 * cofhe_hip_divfloor_plain_records calls invalid or one above `rows`: it gives zero results and sets the division bit (4) of
 * cofhe_hip_device_status.  COFHE_HIP_EINVAL, nothing written, checked before a pointer is looked at: kbits = 0 or kbits >
 * COFHE_HIP_DIV_MAX_KBITS; rows = 0 or rows > COFHE_HIP_DIVX_MAX_ROWS; n_div = 0; n no multiple of n_div; then an output
 * overlapping an input.  n = 0 does nothing. */
#define COFHE_HIP_DIVX_MAX_ROWS 4096
/* q[e] = floor(s(v[e]) / D) mod 2^kbits as an exponent record and rem[e] = s(v[e]) - D q(v[e]) in [0, D) as a uint32_t, D =
 * div[e mod n_div], e < n: cofhe_hip_divfloor_plain_records that keeps the remainder, one 8-lane limb group per element.  An
 * invalid divisor gives quotient 0 and remainder 0.  One launch ("k_plain_divmod" under "profile_kernels"), purely stream-ordered:
 * no workspace, no read-back, no lock. */
int cofhe_hip_divmod_plain_records(cofhe_hip_ctx *ctx, const void *d_v, const void *d_div, uint64_t n_div, void *d_q, void *d_rem, uint64_t n,
                                   uint32_t rows, uint32_t kbits, void *stream);
/* the plaintext rows: out[i rows + j] = T_j of element i for j < D_i = div[i mod n_div] and the zero record for D_i <= j < rows,
 * i < n, exponent records in [0, 2^kbits) with sign word 0, every word written.  d_r: n records of the masks; d_out: n rows
 * records.  Two launches: "k_divx_prep", one limb group per element, leaves q(r), q(r) + 1 and the threshold D - m(r) in a block of
 * the block cache (it goes back behind the work queued on `stream`), and "k_divx_rows" stores the rows from it, 16-byte pieces
 * when d_out allows them and 4-byte ones otherwise.  An invalid divisor gives `rows` zero records.  No read-back. */
int cofhe_hip_divx_rows_records(cofhe_hip_ctx *ctx, const void *d_r, const void *d_div, uint64_t n_div, void *d_out, uint64_t n, uint32_t rows,
                                uint32_t kbits, void *stream);
/* the tuples' entries: out[i rows + j] = (h^rho, pk^rho o f^(T_j)) with rho = rho[i rows + j] and T the rows of
 * cofhe_hip_divx_rows_records, which it runs into a block of the block cache; then cofhe_hip_encrypt_fresh_records over the n rows
 * plaintexts, whose bytes these are (the plan "comb", kind 1, and its one read-back of the longest exponent).  d_rho: n rows
 * exponent records of the caller's randomness, each used once; h_record, pk_record, f_record: HOST records.  Also
 * COFHE_HIP_EINVAL: kbits out of the comb's range. */
int cofhe_hip_divx_tuples_records(cofhe_hip_ctx *ctx, const void *d_r, const void *d_div, uint64_t n_div, const void *d_rho,
                                  const uint32_t *h_record, const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n,
                                  uint32_t rows, uint32_t kbits, void *stream);
/* The closing step: out[i] = (c1, c2 o f^(q(e[i]))) of tuples[i rows + m(e[i])], i < n, an encryption of floor(s(x[i]) / D_i) when
 * the tuple is the element's and e[i] = x[i] - r (see above).  d_e: n exponent records; d_div: n_div; d_tuples: n rows
 * ciphertexts; f_record: HOST record of f.  Three steps on `stream`: cofhe_hip_divmod_plain_records into a block of the block
 * cache, the copy of the named entries ("k_divx_select" under "profile_kernels": one wavefront per ciphertext, the entry index
 * in 64 bits, never beyond the element's tuple), and the plaintext addend of cofhe_hip_add_plain_records (mode 0, no randomness)
 * against the cached table of f.  Uses the block cache and, through the addend, the workspace plan "comb" (kind 3).  No
 * read-back.  It has no serialised twin: Engine.divx_close_tensors_bytes composes one as Engine.lut_select_tensors_bytes does. */
int cofhe_hip_divx_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_div, uint64_t n_div, const void *d_tuples, uint32_t rows,
                                 const uint32_t *f_record, void *d_out, uint64_t n, uint32_t kbits, void *stream);
/* host only, no GPU: *rows of the tuples that go with opened values of shape shape_e[ndim_e], ndim_e <= 7.  COFHE_HIP_ESHAPE unless
 * shape_t is shape_e with one more, last dimension of `rows` entries, 1 <= rows <= COFHE_HIP_DIVX_MAX_ROWS. */
int cofhe_hip_divx_shape(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t *rows);
/* ---- table lookups from one opened value (cofhe_amd/csrc/lut.hip) ----
 * For values known to lie in a b-bit range, 1 <= b <= COFHE_HIP_LUT_MAX_BITS, b <= k, ANY public function of them given as a table
 * g of 2^b plaintexts is evaluated exactly, in one round, with no failure probability.  A LOOKUP TUPLE of an element is
 * ([r], [T_0], .., [T_{2^b - 1}]) with r uniform in Z/2^k and T_j = g[(j + r) mod 2^b], used once.  With the ONE opened value
 * e = Dec([x] - [r]) -- uniform whatever x is, so it hides x perfectly --
 *   [y] = [T_{e mod 2^b}],   y = g[x mod 2^b],
 * since (e + r) mod 2^b = x mod 2^b: the closing step is a copy, no homomorphic arithmetic.  A b-bit SIGNED value is read as its
 * two's-complement index: the caller's choice of g.  EVERY [T_j] MUST CARRY ITS OWN RANDOMNESS: under one shared r the quotient
 * c2_j o c2_j'^-1 = f^(T_j - T_j') is publicly decodable, which reveals the rotation and, with e, x mod 2^b; so the tuples are made
 * by the fresh-randomness comb (cofhe_hip_lut_tuples_records) and by nothing else.  A tuple is 2^b * 1344 bytes per element.
 * "The index of a record" below: the low b bits of its value mod 2^k, read from word 0 and the sign word -- m mod 2^b, or
 * (2^b - m mod 2^b) mod 2^b under a set sign word; -0 and magnitudes of 2^k and above follow the same rule.
 * All three records entry points: purely stream-ordered, no read-back of their own; 16-byte accesses when the pointers allow them,
 * 4-byte ones otherwise.  COFHE_HIP_EINVAL, nothing written: bits = 0 or bits > COFHE_HIP_LUT_MAX_BITS; n_tab = 0; n no multiple of
 * n_tab; an output overlapping an input.  n = 0 does nothing. */
#define COFHE_HIP_LUT_MAX_BITS 12
/* the plaintext rows: out[i 2^bits + j] = table[(i mod n_tab) 2^bits + ((j + r[i]) mod 2^bits)], i < n, j < 2^bits, exponent records
 * copied word for word.  d_table: n_tab 2^bits records (n_tab = 1: one table; n: one per element); d_r: n records, of which the
 * index is used; d_out: n 2^bits records.  One launch ("k_lut_rotate" under "profile_kernels"), no workspace, no lock. */
int cofhe_hip_lut_rotate_records(cofhe_hip_ctx *ctx, const void *d_table, uint64_t n_tab, const void *d_r, void *d_out, uint64_t n,
                                 uint32_t bits, void *stream);
/* the tuples' entries: out[i 2^bits + j] = (h^rho, pk^rho o f^(T_j mod 2^kbits)) with rho = rho[i 2^bits + j] and T the rows of
 * cofhe_hip_lut_rotate_records, which it runs into a block of the block cache (it goes back behind the work queued on `stream`);
 * then cofhe_hip_encrypt_fresh_records over the n 2^bits plaintexts, whose bytes these are (the plan "comb", kind 1, and its one
 * read-back of the longest exponent).  d_rho: n 2^bits exponent records of the caller's randomness, each used once; h_record,
 * pk_record, f_record: HOST records.  Also COFHE_HIP_EINVAL: bits > kbits, kbits out of the comb's range. */
int cofhe_hip_lut_tuples_records(cofhe_hip_ctx *ctx, const void *d_table, uint64_t n_tab, const void *d_r, const void *d_rho,
                                 const uint32_t *h_record, const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n,
                                 uint32_t bits, uint32_t kbits, void *stream);
/* The closing step: out[i] = tuples[i 2^bits + (e[i] mod 2^bits)], i < n, ciphertexts of 1344 bytes copied byte for byte, one
 * wavefront each.  d_e: n exponent records of the opened values x - r; d_tuples: n 2^bits ciphertexts; d_out: n.  One launch
 * ("k_lut_select" under "profile_kernels"), no workspace, no lock.  The result is a fresh ciphertext already: a caller in
 * per-element randomness mode has nothing to re-randomise.  It has NO serialised twin (no cofhe_hip_lut_select_tensors_bytes):
 * tensors that arrive as bytes go through cofhe_hip_unpack_tensor_device (kind 0 for e of shape S, kind 2 for the tuples of shape
 * S + [2^bits]; it validates the incoming forms), cofhe_hip_lut_tuples_shape_bits, this call and cofhe_hip_pack_tensor_device, as
 * Engine.lut_select_tensors_bytes does. */
int cofhe_hip_lut_select_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_tuples, void *d_out, uint64_t n, uint32_t bits,
                                 void *stream);
/* host only, no GPU: *bits of the tuples that go with opened values of shape shape_e[ndim_e], ndim_e <= 7.  COFHE_HIP_ESHAPE unless
 * shape_t is shape_e with one more, last dimension of 2^bits entries, 1 <= bits <= COFHE_HIP_LUT_MAX_BITS. */
int cofhe_hip_lut_tuples_shape_bits(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t *bits);
/* ---- the sign on a window of up to 64 bits from digit comparisons (cofhe_amd/csrc/compare.hip, compare.hpp) ----
 * For values known to lie in the signed window of l = bits bits, 2 <= l <= min(k, 64), the sign is computed exactly in two rounds
 * with a tuple that grows with (l / d) 2^d, not 2^l.  r mod 2^l is read as n = ceil(l / d) digits r_j of d = digit_bits bits, 1 <=
 * d <= COFHE_HIP_CMP_MAX_DIGIT_BITS, n + 1 <= min(COFHE_HIP_LUT_MAX_BITS, k).  A COMPARISON TUPLE of an element is ([r], [T]) with r
 * uniform in Z/2^k and T[j][c] = 2^j sgn(r_j - c) mod 2^k, j < n, c < 2^d (every digit has 2^d entries, also the top one when d
 * does not divide l), used once.  Round 1 opens e = Dec([x] - [r]); with u = e mod 2^l, x < 0 exactly when r mod 2^l lies in the
 * cyclic interval [A, B), A = (2^(l-1) - u) mod 2^l, B = -u mod 2^l, so [x < 0] = [r >= A] - [r >= B] + wrap, wrap = [A > B] public.
 * For a public threshold t, S_t = sum_j 2^j sgn(r_j - t_j) lies in (-2^n, 2^n) and [r >= t] = [S_t >= 0]; [S_t] = prod_j [T[j][t_j]].
 * A and B differ in the top digit only.  Round 2 is one lookup (above) of n + 1 bits over the 2 E values [S_A], [S_B] with the
 * table g[v] = 1 for v < 2^n, 0 otherwise: [x >= 0] = (1 - wrap) - g(S_A) + g(S_B).  EVERY T[j][c] MUST CARRY ITS OWN RANDOMNESS, for
 * the reason given for the lookups.  A tuple is n 2^d * 1344 bytes per element.
 * "u of a record" below: the low l bits of its value mod 2^k, read from words 0 and 1 and the sign word -- the 64-bit two's
 * complement of the two words under a set sign word; -0 and magnitudes of 2^k and above follow the same rule.
 * The records entry points: stream-ordered, no read-back of their own; 16-byte accesses where the pointers allow them, 4-byte ones
 * otherwise.  COFHE_HIP_EINVAL, nothing written: bits < 2, bits > 64, bits > kbits; digit_bits = 0 or > 8; n + 1 >
 * min(COFHE_HIP_LUT_MAX_BITS, kbits); kbits out of range; an output overlapping an input.  n = 0 does nothing. */
#define COFHE_HIP_CMP_MAX_BITS 64
#define COFHE_HIP_CMP_MAX_DIGIT_BITS 8
/* the plaintext rows: out[(i nd + j) 2^d + c] = 2^j sgn(r_ij - c), i < n, j < nd = ceil(bits / d), c < 2^d, exponent records: the
 * magnitude in word 0, a set sign word for a negative entry, an all-zero record for equality.  d_r: n records, of which u is
 * used; d_out: n nd 2^d records.  One launch ("k_cmp_rows" under "profile_kernels"), no workspace, no lock. */
int cofhe_hip_cmp_rows_records(cofhe_hip_ctx *ctx, const void *d_r, void *d_out, uint64_t n, uint32_t bits, uint32_t digit_bits,
                               uint32_t kbits, void *stream);
/* the tuples' entries: out[q] = (h^rho, pk^rho o f^(T_q mod 2^kbits)) with rho = rho[q], q < n nd 2^d, and T the rows of
 * cofhe_hip_cmp_rows_records, which it runs into a block of the block cache; then cofhe_hip_encrypt_fresh_records over the
 * n nd 2^d plaintexts, whose bytes these are (the plan "comb", kind 1, and its one read-back of the longest exponent).  d_rho:
 * n nd 2^d exponent records of the caller's randomness, each used once; h_record, pk_record, f_record: HOST records.  Also
 * COFHE_HIP_EINVAL: kbits out of the comb's range. */
int cofhe_hip_cmp_tuples_records(cofhe_hip_ctx *ctx, const void *d_r, const void *d_rho, const uint32_t *h_record,
                                 const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n, uint32_t bits,
                                 uint32_t digit_bits, uint32_t kbits, void *stream);
/* The closing step of round 1: out[2 i + s] = prod_{j < nd} tuples[(i nd + j) 2^d + digit j of t_s], t_0 = A and t_1 = B of
 * u = u of e[i], i < n, ciphertexts; wrap[i] = [A > B] as an exponent record.  d_e: n exponent records of the opened values x - r;
 * d_tuples: n nd 2^d ciphertexts, read in place; d_out: 2 n ciphertexts, [S_A] then [S_B] of each element; d_wrap: n exponent
 * records.  One launch ("k_cmp_close" under "profile_kernels"): one limb group per element and half, the prefix below the top
 * digit composed once, nd compositions each (nd = 1: two copies).  The results share their randomness with the entries they
 * are products of, which are used once.  A composition that fails sets the device status word as everywhere.  No workspace.  It
 * has NO serialised twin: tensors that arrive as bytes go through cofhe_hip_unpack_tensor_device (kind 0 for e of shape S, kind 2
 * for the tuples of shape S + [nd, 2^d]; it validates the incoming forms), cofhe_hip_cmp_shape, this call and
 * cofhe_hip_pack_tensor_device, as Engine.cmp_close_tensors_bytes does. */
int cofhe_hip_cmp_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_tuples, void *d_out, void *d_wrap, uint64_t n,
                                uint32_t bits, uint32_t digit_bits, uint32_t kbits, void *stream);
/* host only, no GPU: *digits = nd = ceil(bits / digit_bits) and *entries = nd 2^digit_bits of one element's tuple (either may be
 * null).  COFHE_HIP_EINVAL for the parameter bounds above.  With shape_t non-null it also validates the tuples that go with
 * opened values of shape shape_e[ndim_e], ndim_e <= 6: COFHE_HIP_ESHAPE unless shape_t is shape_e with two more, last dimensions
 * [nd, 2^digit_bits].  shape_t null (ndim_t ignored): the parameters only. */
int cofhe_hip_cmp_shape(uint32_t bits, uint32_t digit_bits, uint32_t kbits, uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t,
                        const uint32_t *shape_t, uint32_t *digits, uint32_t *entries);
/* ---- rearranging resident tensors: affine views and index gathers (cofhe_amd/csrc/view.hip, view.hpp) ----
 * Pure data movement on records of `words` dwords each (336 a ciphertext, 168 a form or a partial decryption, 32 an exponent
 * record): every record of the result is a byte-for-byte copy of a source record or of the fill record.  No composition runs and
 * nothing is re-randomised: A COPY SHARES ITS RANDOMNESS WITH ITS SOURCE, so c2 o c2'^-1 of a copy and its original is the
 * principal form; a caller that hands both to another party re-randomises one of them first (cofhe_hip_rerandomize_records).
 *
 * An AFFINE VIEW maps an output coordinate to a source coordinate.  It produces a box of out_extent elements (out_ndim axes; 0
 * axes: one element) from a dense row-major source of src_extent (src_ndim axes): for the output coordinate o the source
 * coordinate on source axis a is c_a = start[a] + sum_d map[a][d] o_d.  Where 0 <= c_a < src_extent[a] holds on every source axis,
 * dst[rowmajor_dst(dst_start + o)] = src[rowmajor_src(c)]; otherwise that destination element receives the fill record.  The box
 * lies at dst_start inside a dense row-major destination of dst_extent (out_ndim axes); destination elements outside the box are
 * not written, which is how K calls concatenate K tensors into one.  One descriptor expresses a permutation of the axes (a
 * permutation matrix), a slice with a step, a flip (-1), a broadcast (a zero column), padding (a negative start), a diagonal (a
 * column with two ones) and sliding windows (two output axes mapped onto one source axis: y = oy sh + dy dh - ph). */
#define COFHE_HIP_VIEW_MAX_DIMS 8
typedef struct {
    uint32_t out_ndim, src_ndim;                 /* 0..8; 0 = one element */
    uint64_t out_extent[8], src_extent[8];       /* the box that is produced; the dense row-major source */
    int64_t start[8];                            /* per SOURCE axis */
    int32_t map[8][8];                           /* map[a][d]: source axis a advances by this per step of output axis d */
    uint64_t dst_extent[8], dst_start[8];        /* the box lies at dst_start inside a dense row-major destination of dst_extent */
} cofhe_hip_view;
#define COFHE_HIP_GATHER_FILL 0xFFFFFFFFu        /* cofhe_hip_gather_records: this output receives the fill record */
#define COFHE_HIP_GATHER_KEEP 0xFFFFFFFEu        /* ... this output is left as it is */
/* host only, no GPU, no context: the element counts of the source, the box and the destination, and *needs_fill = 1 when some
 * element of the box can read outside the source (exact: the range of every c_a over the box, by interval arithmetic in 128 bits).
 * Any output pointer may be null.  COFHE_HIP_EINVAL: more than 8 axes; a box that does not lie inside dst_extent; a c_a that can
 * leave the range of an int64; more than 2^48 elements in the source, the box or the destination.  A zero extent is legal and
 * gives a count of 0. */
int cofhe_hip_view_check(const cofhe_hip_view *view, uint64_t *n_src, uint64_t *n_box, uint64_t *n_dst, int *needs_fill);
/* host only: the builders fill *view for a dense row-major source of shape[ndim], ndim <= 8, and set dst_extent = out_extent,
 * dst_start = 0.  COFHE_HIP_EINVAL for a null pointer, more than 8 axes and what each names below.
 * permute: output axis d is source axis perm[d] (numpy.transpose); perm must be a permutation of 0 .. ndim - 1.
 * slice: out = src[start[0]:stop[0]:step[0], ...] with numpy's meaning for bounds given in range: step != 0; with step > 0,
 *   0 <= start <= shape and 0 <= stop <= shape; with step < 0, -1 <= stop and start <= shape - 1, where a stop of -1 stands for
 *   "down to and including element 0" (numpy's None).  An empty range gives an extent of 0.  |step| < 2^31.
 * pad: out extent lo + shape + hi, the source at offset lo; the elements around it receive the fill record.
 * broadcast: numpy's rule, right-aligned: every source extent equals the output extent it is aligned with, or is 1.
 * window_taps: [B, H, W, C] -> [kh, kw, B, Ho, Wo, C], out[dy, dx, b, oy, ox, c] = src[b, oy sh + dy dh - ph, ox sw + dx dw - pw, c]
 *   or the fill record in the padding, with the extents and the refusals of cofhe_hip_conv2d_geometry_out_shape; Co and groups
 *   are ignored.
 * into: places the box of an existing descriptor at dst_start inside a destination of dst_shape (out_ndim axes each). */
int cofhe_hip_view_permute(const uint64_t *shape, uint32_t ndim, const uint32_t *perm, cofhe_hip_view *view);
int cofhe_hip_view_slice(const uint64_t *shape, uint32_t ndim, const int64_t *start, const int64_t *stop, const int64_t *step,
                         cofhe_hip_view *view);
int cofhe_hip_view_pad(const uint64_t *shape, uint32_t ndim, const uint64_t *lo, const uint64_t *hi, cofhe_hip_view *view);
int cofhe_hip_view_broadcast(const uint64_t *shape, uint32_t ndim, const uint64_t *out_shape, uint32_t out_ndim, cofhe_hip_view *view);
int cofhe_hip_view_window_taps(const cofhe_hip_conv2d_geometry *geometry, cofhe_hip_view *view);
int cofhe_hip_view_into(cofhe_hip_view *view, const uint64_t *dst_shape, const uint64_t *dst_start);
/* The view on the device: purely stream-ordered, no read-back, no workspace, no lock; one launch ("k_view_records" under
 * "profile_kernels"), none when the box is empty.  d_src: n_src records; d_fill: ONE record, may be null when the view needs no
 * fill; d_dst: n_dst records, of which the n_box of the box are written.  16-byte accesses when the three pointers and the record
 * size allow them, 4-byte ones otherwise.  Records of 64 pieces or more are moved by one wavefront each, shorter ones by eight lanes
 * each; the grid strides beyond 64 workgroups per CU ("view_grid_blocks" pins the grid).  The status word is not touched.
 * COFHE_HIP_EINVAL, nothing written: a descriptor that cofhe_hip_view_check refuses; a fill is needed and d_fill is null; words =
 * 0; the destination overlaps the source or the fill. */
int cofhe_hip_view_records(cofhe_hip_ctx *ctx, const cofhe_hip_view *view, const void *d_src, const void *d_fill, void *d_dst,
                           uint32_t words, void *stream);
/* dst[i] = src[index[i]], i < n_out: d_index holds n_out uint32_t on the device.  COFHE_HIP_GATHER_FILL writes the fill record,
 * COFHE_HIP_GATHER_KEEP leaves dst[i] untouched (several source blocks are gathered into one destination by one call each, with
 * KEEP at the other blocks' elements).  Any other index >= n_src writes the fill record -- or, with d_fill null, leaves dst[i]
 * untouched -- and sets bit 32 of the device status word; nothing is ever read out of range.  d_fill may be null when no index is
 * FILL (a FILL index is then treated like KEEP).  One launch ("k_gather_records"), none for n_out = 0; the lane mapping, the access
 * width and "view_grid_blocks" as above.  COFHE_HIP_EINVAL, nothing written: words = 0; n_src > 0xFFFFFFFE; the destination
 * overlaps the source, the indices or the fill. */
int cofhe_hip_gather_records(cofhe_hip_ctx *ctx, const void *d_src, uint64_t n_src, const void *d_index, const void *d_fill, void *d_dst,
                             uint64_t n_out, uint32_t words, void *stream);
/* ---- piecewise-polynomial activations from one opened value (cofhe_amd/csrc/spline.hip) ----
 * A SPLINE TABLE over a window of W = shift + bits <= k bits is 2^bits pieces of d + 1 plaintext coefficients, 1 <= d <=
 * COFHE_HIP_POLY_MAX_DEGREE, 2^bits (d + 1) <= COFHE_HIP_SPLINE_MAX_TUPLE.  Piece p has the origin o(p) = sigma(p) 2^shift, sigma(p) the
 * bits-bit two's-complement reading of p, and evaluates S_p(x) = sum_i c[p][i] (x - o(p))^i mod 2^k; the segment of x is
 * seg(x) = floor((x mod 2^W) / 2^shift).  A SPLINE TUPLE of an element is ([r], [q_{j,i}], j < 2^bits, i <= d), used once: r uniform in
 * Z/2^k, rho = seg(r), p_j = (j + rho) mod 2^bits, and q_{j,.} the Taylor shift of piece p_j at (r - o(p_j)) mod 2^k, that is
 * sum_i q_{j,i} E^i = sum_i c[p_j][i] (E + r - o(p_j))^i.  With the ONE opened value e = Dec([x] - [r]) -- uniform whatever x is, so
 * it hides x perfectly -- and j = seg(e),
 *   [y] = [q_{j,0}] o prod_{i=1..d} [q_{j,i}]^(e^i mod 2^k),   y = S_{p'}(x) mod 2^k,   p' = (seg(x) - c) mod 2^bits,
 * c = [(e mod 2^shift) + (r mod 2^shift) >= 2^shift]: the element's own piece or the one below (the carry of the low shift bits is
 * lost, as in the division's "floor quotient or one less"; the wrap of k never matters, since 2^W divides 2^k).  The tuple holds
 * 2^bits (d + 1) ciphertexts where a lookup over the same window holds 2^(shift + bits).  THE CALLER'S CONTRACT: piece p approximates
 * the function on [o(p), o(p) + 2^(shift + 1)), two segments; x stays out of the lowest segment (sigma = -2^(bits - 1)), where the
 * piece below wraps round to the top piece; fixed-point scales are the caller's, as for the polynomials.  shift = 0 has no carry:
 * the result is exact on the element's own piece.  EVERY [q_{j,i}] MUST CARRY ITS OWN RANDOMNESS, for the reason given for the
 * lookups: under a shared c1 the quotients of the c2 are publicly decodable and give the rotation away; so the tuples are made by
 * the fresh-randomness comb (cofhe_hip_spline_tuples_records) and by nothing else.  The reference has no such operation.
 * "The segment of a record" below: bits shift .. shift + bits - 1 of its value mod 2^k (sign word honoured, -0 and magnitudes of
 * 2^k and above reduced, as in cofhe_hip_matmul_plain_plain_records); the field may straddle a word and lie in any word.
 * All three records entry points: stream-ordered, no read-back of their own.  COFHE_HIP_EINVAL, nothing written: bits = 0; d = 0 or
 * d > COFHE_HIP_POLY_MAX_DEGREE; 2^bits (d + 1) > COFHE_HIP_SPLINE_MAX_TUPLE; shift + bits > kbits; kbits outside 1 .. 639; n_tab = 0;
 * n no multiple of n_tab; an output overlapping an input.  n = 0 does nothing. */
#define COFHE_HIP_SPLINE_MAX_TUPLE 4096
/* the plaintext rows: out[(i 2^bits + j) (d + 1) + c] = q_{j,c} of element i, i < n, j < 2^bits, c <= d, exponent records in
 * [0, 2^kbits) with sign word 0.  d_pieces: n_tab tables of 2^bits (d + 1) records, piece-major (n_tab = 1: one table; n: one per
 * element; element i reads table i mod n_tab); d_r: n records.  One launch ("k_spline_rows" under "profile_kernels"), one thread
 * per element and row, no workspace, no lock. */
int cofhe_hip_spline_rows_records(cofhe_hip_ctx *ctx, const void *d_pieces, uint64_t n_tab, const void *d_r, void *d_out, uint64_t n,
                                  uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits, void *stream);
/* the tuples' entries: out[m] = (h^rho[m], pk^rho[m] o f^(row[m])) with row the output of cofhe_hip_spline_rows_records, which it runs
 * into a block of the block cache (it goes back behind the work queued on `stream`); then cofhe_hip_encrypt_fresh_records over the
 * n 2^bits (d + 1) plaintexts, whose bytes these are (the plan "comb", kind 1, and its one read-back of the longest exponent).
 * d_rho: n 2^bits (d + 1) exponent records of the caller's randomness, each used once; h_record, pk_record, f_record: HOST records. */
int cofhe_hip_spline_tuples_records(cofhe_hip_ctx *ctx, const void *d_pieces, uint64_t n_tab, const void *d_r, const void *d_rho,
                                    const uint32_t *h_record, const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n,
                                    uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits, void *stream);
/* the powers of the opened values: out[(c - 1) n + i] = e[i]^c mod 2^kbits, c = 1 .. d, i < n, exponent records in [0, 2^kbits) with
 * sign word 0, power-major: the layout cofhe_hip_pow_dot_records reads its exponents in.  One launch ("k_spline_powers" under
 * "profile_kernels"), one thread per element, no workspace, no lock.  COFHE_HIP_EINVAL: d = 0 or d > COFHE_HIP_POLY_MAX_DEGREE,
 * kbits outside 1 .. 639, d_out overlapping d_e. */
int cofhe_hip_spline_powers_records(cofhe_hip_ctx *ctx, const void *d_e, void *d_out, uint64_t n, uint32_t d, uint32_t kbits, void *stream);
/* The closing step: out[i] = [q_{j,0}] o prod_{c=1..d} [q_{j,c}]^(e[i]^c mod 2^kbits), j the segment of e[i], i < n.  d_e: n exponent
 * records of the opened values x - r; d_tuples: n 2^bits (d + 1) ciphertexts; d_out: n.  Two launches: cofhe_hip_spline_powers_records
 * into a block of the block cache (which goes back behind the work queued on `stream`), and "k_spline_close", which runs the walk
 * of cofhe_hip_pow_dot_records with the bases read in place from row j of the element's tuple -- no gather copy -- and
 * [q_{j,0}] as the last composition of every record; e[i] = 0 gives [q_{j,0}] itself.  A sequence kernel: it reports
 * through cofhe_hip_device_status.  It has NO serialised twin: tensors that arrive as bytes go through
 * cofhe_hip_unpack_tensor_device (kind 0 for e of shape S, kind 2 for the tuples of shape S + [2^bits, d + 1]; it validates the
 * incoming forms), cofhe_hip_spline_tuples_shape, this call and cofhe_hip_pack_tensor_device, as Engine.spline_close_tensors_bytes
 * does. */
int cofhe_hip_spline_close_records(cofhe_hip_ctx *ctx, const void *d_e, const void *d_tuples, void *d_out, uint64_t n, uint32_t bits,
                                   uint32_t shift, uint32_t d, uint32_t kbits, void *stream);
/* host only, no GPU: *bits and *d of the tuples that go with opened values of shape shape_e[ndim_e], ndim_e <= 6.  COFHE_HIP_ESHAPE
 * (and *bits, *d left alone) unless shape_t is shape_e with two more, last dimensions [2^bits, d + 1], bits >= 1, 1 <= d <=
 * COFHE_HIP_POLY_MAX_DEGREE, 2^bits (d + 1) <= COFHE_HIP_SPLINE_MAX_TUPLE. */
int cofhe_hip_spline_tuples_shape(uint32_t ndim_e, const uint32_t *shape_e, uint32_t ndim_t, const uint32_t *shape_t, uint32_t *bits,
                                  uint32_t *d);
/* decryption: for each of n ciphertexts, m with c2 o (c1^sk)^-1 = f^m.  sk: one exponent record on
 * the device; f_record: HOST pointer to the 168-word record of f = (2^(2k), 2^(k+1), 1 - Delta_K)
 * (its table of f^(-2^j) is built on first use and cached in the context).  d_out receives
 * ceil(k/32) little-endian words of m followed by one status word (0 ok, 1 = not in <f>) per
 * ciphertext.  Reference: CL_HSM2k::decrypt via cpu_cryptosystem_tensor_ops.inl:21-33.
 * When all n >= 64 ciphertexts carry the same c1 (a tensor made by encrypt_tensor, or a sum of such tensors) c1^sk is
 * computed once and copied; tensors with differing c1 run one ladder per ciphertext.  Same for part_decrypt below. */
int cofhe_hip_decrypt_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_sk, const uint32_t *f_record,
                              void *d_out, uint64_t n_ciphertexts, uint32_t kbits, void *stream);
/* out[i,k] = zero o prod_j x[i,j,k]: x is n x m x p ciphertexts (row-major), zero 1 ciphertext, out n x p.
 * The accumulation loop of the ciphertext x ciphertext matrix product,
 * include/smpc/ciphertext_multiplications.hpp:85-101. */
int cofhe_hip_accumulate_records(cofhe_hip_ctx *ctx, const void *d_x, const void *d_zero, void *d_out, uint32_t n,
                                 uint32_t m, uint32_t p, void *stream);
/* out[i] = base[i] ^ exp[i] on single forms (n_forms records, n_forms exponent records) */
int cofhe_hip_pow_form_records(cofhe_hip_ctx *ctx, const void *d_base, const void *d_exp, void *d_out,
                               uint64_t n_forms, void *stream);
/* out = base^e for a base that recurs (h of the cryptosystem, a public key): base_record and exp_record are HOST
 * pointers (168 / 32 words), d_out one form record on the device.  The context keeps the table base^(2^j) of the last
 * few bases (first use of a base: one chain of ~1000 squarings, ~0.5 s); afterwards the power is a product tree over
 * the ~bits/3 entries the signed binary digits of e select -- a few milliseconds.  Reference: h^r and pk^r of
 * encrypt_tensor, cpu_cryptosystem_tensor_ops.inl:7-12; h^sk of keygen, cpu_cryptosystem.inl:6-9. */
int cofhe_hip_pow_fixed_base_record(cofhe_hip_ctx *ctx, const uint32_t *base_record, const uint32_t *exp_record, void *d_out,
                                    void *stream);
/* n <= 4 such powers at once (base_records: n x 168 words, exp_records: n x 32 words, both HOST; d_out: n records):
 * one gather and one product tree for all of them, so h^r and pk^r of an encryption cost one tree's latency. */
int cofhe_hip_pow_fixed_base_records(cofhe_hip_ctx *ctx, uint32_t n, const uint32_t *base_records, const uint32_t *exp_records,
                                     void *d_out, void *stream);
/* encryption with given randomness: out[e] = (c1, pk^r o f^(m_e mod 2^k)).  d_plain: n exponent records
 * (plaintexts, sign honoured); d_c1_pkr: 2 form records on the device, c1 = h^r then pk^r (two powers the
 * caller takes once per tensor with cofhe_hip_pow_form_records); f_record as for decryption (the same cached
 * table of f^(-2^j) serves as the fixed-base table).  Reference: encrypt_tensor,
 * cpu_cryptosystem_tensor_ops.inl:1-19 (one r per tensor, element i = CipherText(hsm2k, m_i, c1, pkr)). */
int cofhe_hip_encrypt_records(cofhe_hip_ctx *ctx, const void *d_plain, const void *d_c1_pkr, const uint32_t *f_record,
                              void *d_out, uint64_t n_ciphertexts, uint32_t kbits, void *stream);
/* ---- fresh randomness per element: the fixed-base comb (cofhe_amd/csrc/comb.hpp) ----
 * A tensor that encrypt_tensor makes shares ONE r (cpu_cryptosystem_tensor_ops.inl:1-19): c2_i o c2_j^-1 = f^(m_i - m_j), and
 * discrete logarithms in <f> are public, so the ciphertexts alone give every plaintext difference mod 2^k.  These entry
 * points give each ciphertext its own r -- the reference's ADD_RANDOMNESS_IN_HOMOMORPHIC_OPERATIONS /
 * DIFFERENT_RANDOMNESS_FOR_EACH_OPERATION branches (cpu_cryptosystem_vector_ops.inl:1-2, tensor_ops.inl:142-162, 212-240,
 * 287-310, 357-375, 431-460), which are compiled out there.  Each power is a product of ~floor(bits/w) + 1 entries of a
 * table T[j][d] = base^(d 2^(wj)) (signed Booth digits, no squarings), cached per (base, w) in the context (w = 8: 10.8 MB;
 * first use of a base: its chain of ~1000 squarings plus w - 1 table levels).  Exponents and plaintexts are exponent
 * records on the device, signs honoured; r = 0 gives the principal form; n = 0 does nothing.  The caller supplies the
 * randomness (r_i < exponent_bound), as for cofhe_hip_encrypt_records.  Options "comb_width" (2..10) and "comb_chunk"
 * (items per pass) pin the launcher's choices; the results do not depend on them.  Each call synchronises `stream` once
 * (the longest exponent sizes the tree: a 4-byte read-back), and its workspace stays within 4 GiB for any n.
 * With "profile_kernels" on, every launch records a span: "k_comb_table" (w - 1 per table built), "k_comb_first" (one per
 * chunk) and "k_compose_pairs" (the levels above). */
/* out[i] = base^e[i]: n exponent records on the device, one HOST base record (any reduced form).  Reference: the nupow of
 * h^r_i and pk^r_i in the branches above (tensor_ops.inl:223-226 asks for exactly this batch). */
int cofhe_hip_pow_fixed_base_many_records(cofhe_hip_ctx *ctx, const uint32_t *base_record, const void *d_exps, void *d_out, uint64_t n,
                                          void *stream);
/* out[i] = (h^r[i], pk^r[i] o f^(m[i] mod 2^k)): encryption with its own randomness per element.  h, pk, f: HOST records.
 * Reference: encrypt_tensor, cpu_cryptosystem_tensor_ops.inl:1-19, with one r per element instead of one per call. */
int cofhe_hip_encrypt_fresh_records(cofhe_hip_ctx *ctx, const void *d_plain, const void *d_r, const uint32_t *h_record,
                                    const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n_ciphertexts,
                                    uint32_t kbits, void *stream);
/* out[i] = (c1[i] o h^r[i], c2[i] o pk^r[i]): re-randomisation (an encryption of 0 added); d_out may equal d_cts.
 * Reference: the re-randomised outputs of add / scal / negate, tensor_ops.inl:142-162, 212-240, 287-310, 357-375, 431-460. */
int cofhe_hip_rerandomize_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_r, const uint32_t *h_record,
                                  const uint32_t *pk_record, void *d_out, uint64_t n_ciphertexts, void *stream);
/* Ciphertext and plaintext tensor combined without an encryption.  mode 0: ct + m, 1: ct - m, 2: m - ct, with m[i]
 * exponent records (sign honoured, reduced mod 2^k).  d_r NULL: deterministic, (c1, c2 o f^(+-m)) -- c1 untouched (mode 2:
 * inverted), one tree of ~k/w + 2 slots per ciphertext against the cached table of f, no read-back: purely stream-ordered
 * (h_record, pk_record unused).  d_r given (with h, pk): the result carries fresh randomness, (c1 o h^r, c2 o pk^r o f^m) in
 * one tree.  f: HOST record; d_out may equal d_cts.  Reference: the node's mixed ADD encrypts the plaintext and adds
 * (include/node/compute_request_handler.hpp:384-403, 452-470): h^r, pk^r, f^m and two compositions per element, and a
 * second c1 in the result. */
int cofhe_hip_add_plain_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_plain, const void *d_r, const uint32_t *h_record,
                                const uint32_t *pk_record, const uint32_t *f_record, void *d_out, uint64_t n_ct, uint32_t kbits, int mode,
                                void *stream);
/* The comb launcher's decisions as data (host only, no GPU): for kind 0 (powers), 1 (fresh encryption), 2
 * (re-randomisation), 3 (plaintext addend: one column per ciphertext, exp_bits unused) or 4 (plaintext addend with fresh
 * randomness) of n items whose longest exponent has exp_bits bits, with the "comb_width" / "comb_chunk" pins
 * w_pin / chunk_pin (0 = automatic): the window width, the slots (tree leaves) of one output record and the items per pass. */
int cofhe_hip_comb_shape(uint32_t kind, uint64_t n, uint32_t exp_bits, uint32_t kbits, uint32_t w_pin, uint64_t chunk_pin, uint32_t *w,
                         uint32_t *slots, uint64_t *chunk);
/* threshold decryption, party side: out[e] = c1[e] ^ share (one form record per ciphertext; d_share: one
 * exponent record on the device).  Reference: partDecrypt, cpu_cryptosystem_distributed.inl:259-269, looped
 * by part_decrypt_tensor, cpu_cryptosystem_tensor_ops.inl:35-48. */
int cofhe_hip_part_decrypt_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_share, void *d_out,
                                   uint64_t n_ciphertexts, void *stream);
/* threshold decryption, combiner side: m with c2 o (prod_i parts[i][e]^lambda[i])^-1 = f^m.  d_parts:
 * n_parts x n_ciphertexts form records, party-major; lambda: HOST array of n_parts coefficients, each +1
 * or -1 (the reference's compute_lambda gives (1, -1, ..., -1)); n_parts <= 64.  Output as
 * cofhe_hip_decrypt_records.  Reference: finalDecrypt / compute_d, cpu_cryptosystem_distributed.inl:231-285,
 * looped by combine_part_decryption_results_tensor, cpu_cryptosystem_tensor_ops.inl:50-73. */
int cofhe_hip_combine_part_decryptions_records(cofhe_hip_ctx *ctx, const void *d_cts, const void *d_parts,
                                               uint32_t n_parts, const int32_t *lambda, const uint32_t *f_record,
                                               void *d_out, uint64_t n_ciphertexts, uint32_t kbits, void *stream);
/* the same compose launch repeated `iters` times between two HIP events on `stream`;
 * *ms_per_launch = elapsed / iters (used by bench.py for the roofline figure) */
int cofhe_hip_time_compose(cofhe_hip_ctx *ctx, const void *d_a, const void *d_b, void *d_out,
                           uint64_t n_records, int iters, void *stream, float *ms_per_launch);

/* How an entry point would carve the context's workspace (host only, no GPU, no context): the launchers take their
 * regions from the same plan functions, so a CPU test can check every offset and size for any operand count.
 *   op "pow_shared"       args: n_ladders, front_bytes        (k_pow_shared: part_decrypt / decrypt's c1^sk)
 *      "decrypt"          args: n_ct, shared_c1 (0 / 1)       (cofhe_hip_decrypt_records: front = one record per ciphertext)
 *      "part_decrypt"     args: n_ct, shared_c1               (cofhe_hip_part_decrypt_records: no front)
 *      "scal_matmul"      args: n, m, p, exp_bits, w, segs
 *      "scal_matmul_tree" args: n, m, p, exp_bits, w          (the product-tree route of the same)
 *      "conv2d"           args: B, H, W, C, kh, kw, Co, sh, sw, ph, pw, exp_bits, w   (the direct route of
 *                         cofhe_hip_conv2d_plain_ct_records: "table" is B H W C 2 2^(w-2) 672 bytes -- the image, not the patches;
 *                         empty at w = 2, where the image itself is the table; the other regions as "scal_matmul_tree" with
 *                         m = kh kw C, p = Co)
 *      "conv2d_grouped"   args: B, H, W, C, kh, kw, Co, sh, sw, ph, pw, dh, dw, groups, exp_bits, w   (the direct route of
 *                         cofhe_hip_conv2d_grouped_plain_ct_records: the table of "conv2d"; the other regions as
 *                         "scal_matmul_tree" with m = kh kw C / groups, p = Co)
 *      "accumulate_tree"  args: n, m, p
 *      "encrypt_chunk"    args: n_elements, kbits
 *      "fixed_base"       args: n_powers, max_entries
 *      "comb"             args: kind, n_items, exp_bits, kbits, w, chunk   (the comb entry points above; w, chunk: 0 = automatic;
 *                         the regions of one pass over the largest chunk, cofhe_hip_comb_shape gives its size)
 * regions[i] = name, byte offset, byte count, in workspace order; *total_bytes = what ensure_workspace is asked for. */
typedef struct {
    char name[24];
    uint64_t offset, bytes;
} cofhe_hip_ws_region;
int cofhe_hip_workspace_plan(const char *op, const uint64_t *args, uint32_t n_args, cofhe_hip_ws_region *regions,
                             uint32_t cap, uint32_t *n_regions, uint64_t *total_bytes);

/* Stream timer: two HIP events on `stream` -- the stream the library's kernels are launched on (a torch.cuda.Event only
 * sees torch's current stream).  start records the first event; stop records the second, waits for it, returns the time
 * between the two in *ms and releases the timer.  bench.py times every secondary figure of its JSON line with this. */
int cofhe_hip_timer_start(cofhe_hip_ctx *ctx, void *stream, void **timer);
int cofhe_hip_timer_stop(cofhe_hip_ctx *ctx, void *timer, void *stream, float *ms);

/* ---- binary tensor format <-> records (host side, no GPU work) ----
 * The format: u32 ndim; u32 shape[ndim]; one u64 per integer -- its byte offset in the body, bit 63 set when the value is not
 * positive --; the body of little-endian magnitudes, bits/8 + 1 bytes each as written, any length as read (missing bytes are
 * zero, bytes beyond the limb plane must be zero).  Bit 63 means "negative" on b of a form and on an exponent, where a flagged
 * zero is the reference's zero and reads as +0.  a and c of a form are positive: zero is refused, and so is bit 63 on a non-zero
 * a or c (the reference's reader would negate it), by these readers and by cofhe_hip_unpack_tensor_device alike:
 * COFHE_HIP_EINVAL, "form coefficient outside the supported range". */
/* ciphertext tensor bytes -> malloc'd record array (free with cofhe_hip_host_free) */
int cofhe_hip_bytes_to_records(const uint8_t *bytes, size_t len, uint32_t *ndim, uint32_t shape[8],
                               uint32_t **records, uint64_t *n_records);
int cofhe_hip_records_to_bytes(const uint32_t *records, uint64_t n_records, uint32_t ndim,
                               const uint32_t *shape, uint8_t **bytes, size_t *len);
/* partial-decryption tensors (one form per element; serialize_part_decryption_result_tensor,
 * cpu_cryptosystem.inl:510-559 / :561-635): the same layout with 3 integers per element */
int cofhe_hip_pdr_bytes_to_records(const uint8_t *bytes, size_t len, uint32_t *ndim, uint32_t shape[8],
                                   uint32_t **records, uint64_t *n_records);
int cofhe_hip_pdr_records_to_bytes(const uint32_t *records, uint64_t n_records, uint32_t ndim,
                                   const uint32_t *shape, uint8_t **bytes, size_t *len);
/* ---- the same formats produced / consumed on the GPU (cofhe_amd/csrc/wire.hip) ----
 * kind: 2 = ciphertext tensor (2 form records per element), 1 = partial-decryption tensor (1 form record),
 * 0 = plaintext tensor (1 exponent record).  d_bytes holds the serialised tensor in device memory (what
 * a caller uploads verbatim from the socket / file); records come out in the layout the kernels use.
 * Both calls synchronise `stream` (the header and the error / length words travel back to the host). */
int cofhe_hip_unpack_tensor_device(cofhe_hip_ctx *ctx, const void *d_bytes, size_t len, int kind, void *d_records,
                                   uint64_t capacity_records, uint32_t *ndim, uint32_t shape[8], uint64_t *n_records,
                                   void *stream);
int cofhe_hip_pack_tensor_device(cofhe_hip_ctx *ctx, const void *d_records, uint64_t n_records, int kind, uint32_t ndim,
                                 const uint32_t *shape, void *d_bytes, size_t capacity, size_t *len, void *stream);
/* upper bound of the serialised size, for sizing d_bytes */
size_t cofhe_hip_packed_size_bound(uint64_t n_records, int kind, uint32_t ndim);
/* plaintext tensor bytes -> exponent records */
int cofhe_hip_bytes_to_exponents(const uint8_t *bytes, size_t len, uint32_t *ndim, uint32_t shape[8],
                                 uint32_t **exps, uint64_t *n_exps);
void cofhe_hip_host_free(void *p);

/* ---- whole operations on host buffers in the reference's binary formats ---- */
int cofhe_hip_add_ciphertext_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *t1, size_t l1,
                                           const uint8_t *t2, size_t l2, uint8_t **out, size_t *outlen);
/* t1 - t2 element-wise: the node's SUBTRACT (compute_request_handler.hpp:67-76, 342-344); shapes must be equal */
int cofhe_hip_sub_ciphertext_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *t1, size_t l1,
                                           const uint8_t *t2, size_t l2, uint8_t **out, size_t *outlen);
/* cts (ciphertext tensor) and pt (plaintext tensor) of equal shape, mode 0: cts + pt, 1: cts - pt, 2: pt - cts,
 * deterministic: the node's mixed ADD / SUBTRACT (compute_request_handler.hpp:384-403, 452-470) without the encryption.
 * f_record: HOST record of f. */
int cofhe_hip_add_plaintext_tensor_bytes(cofhe_hip_ctx *ctx, const uint8_t *cts, size_t lc, const uint8_t *pt, size_t lp,
                                         const uint32_t *f_record, uint32_t kbits, int mode, uint8_t **out, size_t *outlen);
/* s (plaintext tensor, n x m) . cts (ciphertext tensor, m x p) -> n x p, from zero (1-element ciphertext tensor): the
 * serialised twin of cofhe_hip_matmul_plain_ct_records.  Incoming forms are validated (COFHE_HIP_EINVAL for a non-form);
 * COFHE_HIP_ESHAPE when an operand is not 2-D or s.shape[1] != cts.shape[0]. */
int cofhe_hip_matmul_plain_ct_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *s, size_t ls, const uint8_t *cts, size_t lc,
                                            const uint8_t *zero, size_t lz, uint8_t **out, size_t *outlen);
/* w (plaintext tensor [kh, kw, C, Co]) over cts (ciphertext tensor [B, H, W, C]) from zero (1-element ciphertext tensor), strides
 * sh, sw and zero padding ph, pw: the serialised twin of cofhe_hip_conv2d_plain_ct_records; the result is the 4-D ciphertext
 * tensor [B, Ho, Wo, Co].  Incoming forms are validated (COFHE_HIP_EINVAL for a non-form, and for the geometry's refusals);
 * COFHE_HIP_ESHAPE when an operand is not 4-D or w.shape[2] != cts.shape[3]. */
int cofhe_hip_conv2d_plain_ct_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *w, size_t lw, const uint8_t *cts, size_t lc,
                                            const uint8_t *zero, size_t lz, uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw,
                                            uint8_t **out, size_t *outlen);
/* the serialised twin of cofhe_hip_conv2d_grouped_plain_ct_records: w is the plaintext tensor [kh, kw, C / groups, Co];
 * COFHE_HIP_ESHAPE when an operand is not 4-D or w.shape[2] != cts.shape[3] / groups */
int cofhe_hip_conv2d_grouped_plain_ct_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *w, size_t lw, const uint8_t *cts, size_t lc,
                                                    const uint8_t *zero, size_t lz, uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw,
                                                    uint32_t dh, uint32_t dw, uint32_t groups, uint8_t **out, size_t *outlen);
/* cofhe_hip_conv2d_ct_filters_records has no serialised twin here: on serialised tensors it is composed from
 * cofhe_hip_unpack_tensor_device (which validates the incoming forms), the records entry and cofhe_hip_pack_tensor_device, as the
 * lookups' and the splines' closing steps are (cofhe_amd/engine.py: Engine.conv2d_ct_filters_tensors). */
/* the serialised twin of cofhe_hip_sum_pool2d_records over kh x kw windows: cts [B, H, W, C] -> [B, Ho, Wo, C] */
int cofhe_hip_sum_pool2d_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *cts, size_t lc, const uint8_t *zero, size_t lz, uint32_t kh,
                                       uint32_t kw, uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw, uint8_t **out, size_t *outlen);
/* the serialised twin of cofhe_hip_poly_close_records: coef a 1-D plaintext tensor [d + 1], e a plaintext tensor of any shape,
 * powers the ciphertext tensor [d, shape of e]; the result is a ciphertext tensor of e's shape.  Incoming forms are validated
 * (COFHE_HIP_EINVAL for a non-form); COFHE_HIP_ESHAPE when the shapes do not fit.  f_record: HOST record of f. */
int cofhe_hip_poly_close_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *coef, size_t lcoef, const uint8_t *e, size_t le,
                                       const uint8_t *powers, size_t lp, const uint32_t *f_record, uint32_t kbits, uint8_t **out,
                                       size_t *outlen);
/* the serialised twin of cofhe_hip_div_close_records: e a plaintext tensor of any shape, div a plaintext tensor of one element, of
 * e's last dimension (1-D: per channel) or of e's shape, rq the ciphertext tensor [r_q] of e's shape; the result is a ciphertext
 * tensor of e's shape.  The divisors are host values here: one that is not in [1, 2^(kbits-1)) is COFHE_HIP_EINVAL.  Incoming
 * forms are validated (COFHE_HIP_EINVAL for a non-form); COFHE_HIP_ESHAPE when the shapes do not fit.  f_record: HOST record of f. */
int cofhe_hip_div_close_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *e, size_t le, const uint8_t *div, size_t ldiv, const uint8_t *rq,
                                      size_t lrq, const uint32_t *f_record, uint32_t kbits, uint8_t **out, size_t *outlen);
/* s: plaintext tensor; 1-D x 1-D -> element-wise, 2-D x 2-D -> matmul (zero: 1-element tensor) */
int cofhe_hip_scal_ciphertext_tensors_bytes(cofhe_hip_ctx *ctx, const uint8_t *s, size_t ls,
                                            const uint8_t *cts, size_t lc, const uint8_t *zero, size_t lz,
                                            uint8_t **out, size_t *outlen);

/* ---- more than one GPU: one process (and one context) per GPU ------------------------------------------------------
 * The path shards by rows with no exchange between chained operations (row i of the result of
 * add_ciphertext_tensors / scal_ciphertext_tensors needs only row i of the ciphertext operand: reference loops
 * cpu_cryptosystem_tensor_ops.inl:242-264, :396-417; the plaintext matrix and Enc(0) are replicated).  The one
 * collective reassembles a row-sharded result: RCCL all-gather of the fixed-size records on the device buffers.
 * The reference has no counterpart (one tensor per compute node); these are additions for the host application.
 *
 * cofhe_hip_shard_rows: rank's contiguous row block [row0, row0 + n_local), remainder rows to the low ranks.
 * cofhe_hip_comm_unique_id: rank 0 draws the id and hands it to the other ranks over the application's own channel.
 * cofhe_hip_comm_create: collective over all ranks (ncclCommInitRank on the context's device).
 * cofhe_hip_all_gather_rows: d_local = this rank's rows (n_local * row_bytes bytes), d_out = all n_rows rows on every
 *   rank; row_bytes = columns * records per element * 672.  Runs on `stream` (the stream of the compute that produced
 *   d_local: the collective is ordered after it with no host synchronisation).  Equal blocks: one ncclAllGather; ragged
 *   blocks: one ncclBroadcast per non-empty block inside a group.
 * cofhe_hip_gather_plan: that decision as data (host only, no GPU, no RCCL): byte offset and byte count of every rank's
 *   block in the assembled tensor, *uniform = 1 for the ncclAllGather route.  offsets / counts: `world` entries each.
 * cofhe_hip_comm_info: world and rank the communicator was made with, and the rank count RCCL reports (ncclCommCount).
 * cofhe_hip_comm_set_option: "force_grouped_broadcast" != 0 takes the ragged route for equal blocks too (testing the
 *   grouped-broadcast branch where the row count happens to divide). */
typedef struct cofhe_hip_comm cofhe_hip_comm;
#define COFHE_HIP_COMM_ID_BYTES 128
void cofhe_hip_shard_rows(uint64_t n_rows, uint32_t world, uint32_t rank, uint64_t *row0, uint64_t *n_local);
int cofhe_hip_comm_unique_id(uint8_t id[COFHE_HIP_COMM_ID_BYTES]);
int cofhe_hip_comm_create(cofhe_hip_ctx *ctx, const uint8_t id[COFHE_HIP_COMM_ID_BYTES], uint32_t world, uint32_t rank,
                          cofhe_hip_comm **out);
void cofhe_hip_comm_destroy(cofhe_hip_comm *comm);
int cofhe_hip_all_gather_rows(cofhe_hip_ctx *ctx, cofhe_hip_comm *comm, const void *d_local, uint64_t n_rows, uint64_t row_bytes,
                              void *d_out, void *stream);
int cofhe_hip_gather_plan(uint64_t n_rows, uint64_t row_bytes, uint32_t world, uint64_t *offsets, uint64_t *counts, int *uniform);
int cofhe_hip_comm_info(cofhe_hip_comm *comm, uint32_t *world, uint32_t *rank, uint32_t *rccl_nranks);
int cofhe_hip_comm_set_option(cofhe_hip_comm *comm, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif
