// hip_cryptosystem.hpp -- C++ host interface of the MI355X engine, source-compatible with the
// part of CoFHE's CPUCryptoSystem that the local benchmark path uses
// (reference: include/x86_64/cpu_cryptosystem.hpp:23-172, include/cofhe.hpp:77-121,
//  benchmarks/local.cpp).  Same nested type names, same method names / argument order /
// by-value returns / raw-pointer ownership, same exception types and messages:
//   std::invalid_argument("Tensor shapes must be equal")            tensor_ops.inl:205
//   std::invalid_argument("Tensors must be 0D, 1D or 2D for now")   tensor_ops.inl:273
//   std::invalid_argument("Vector sizes must be equal")             tensor_ops.inl:284
//   std::runtime_error("Not implemented")                           tensor_ops.inl:96,120
// All class-group arithmetic runs on the GPU through the C ABI in include/cofhe_hip.h; this
// header only moves GMP integers into limb records and back.  GMP is used here exactly as the
// reference's own value types use it (BICYCL::Mpz wraps mpz_t): as the host number container.
//
// Not on this path: the network layer.
#pragma once
#include <gmp.h>

#include <array>
#include <atomic>
#include <cstdint>
#include <memory>
#include <sstream>
#include <cstring>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cofhe_hip.h"
// host-side packing loops can run under OpenMP like the reference's CoFHE_PARALLEL_FOR_STATIC_SCHEDULE
// loops (cpu_cryptosystem_tensor_ops.inl:242) -- opt-in with -DCOFHE_HOST_OPENMP -fopenmp and a sensible
// OMP_NUM_THREADS: on a 16-core share of a 128-core host the default team size made the 64x64 harness
// 40x slower (malloc contention in the per-element `new`), so the shipped harness builds without it
#if defined(_OPENMP) && defined(COFHE_HOST_OPENMP)
#define COFHE_HOST_PARALLEL_FOR _Pragma("omp parallel for schedule(static)")
#else
#define COFHE_HOST_PARALLEL_FOR
#endif
#include "tensor.hpp"

namespace CoFHE {

using String = std::string;
template <typename T>
using Vector = std::vector<T>;

enum class Device { CPU, GPU };

// ---- value types (host containers; no arithmetic beyond what encoding needs) ---------------
class Mpz {
  public:
    Mpz() { mpz_init(z_); }
    Mpz(unsigned long v) { mpz_init_set_ui(z_, v); }
    explicit Mpz(const std::string &dec) { mpz_init_set_str(z_, dec.c_str(), 10); }
    Mpz(const Mpz &o) { mpz_init_set(z_, o.z_); }
    Mpz(Mpz &&o) noexcept { mpz_init(z_); mpz_swap(z_, o.z_); }
    Mpz &operator=(const Mpz &o) { if (this != &o) mpz_set(z_, o.z_); return *this; }
    Mpz &operator=(Mpz &&o) noexcept { mpz_swap(z_, o.z_); return *this; }
    ~Mpz() { mpz_clear(z_); }
    int sgn() const { return mpz_sgn(z_); }
    void neg() { mpz_neg(z_, z_); }
    size_t nbits() const { return mpz_sgn(z_) == 0 ? 0 : mpz_sizeinbase(z_, 2); }
    operator mpz_srcptr() const { return z_; }
    mpz_ptr get() { return z_; }
    mpz_srcptr get() const { return z_; }
    std::string str() const {
        char *s = mpz_get_str(nullptr, 10, z_);
        std::string r(s);
        void (*freefn)(void *, size_t);
        mp_get_memory_functions(nullptr, nullptr, &freefn);
        freefn(s, strlen(s) + 1);
        return r;
    }
    bool operator==(const Mpz &o) const { return mpz_cmp(z_, o.z_) == 0; }

  private:
    mpz_t z_;
};

class QFI {
  public:
    QFI() = default;
    QFI(Mpz a, Mpz b, Mpz c) : a_(std::move(a)), b_(std::move(b)), c_(std::move(c)) {}
    const Mpz &a() const { return a_; }
    const Mpz &b() const { return b_; }
    const Mpz &c() const { return c_; }
    bool operator==(const QFI &o) const { return a_ == o.a_ && b_ == o.b_ && c_ == o.c_; }

  private:
    Mpz a_, b_, c_;
};

// A block of ciphertext records living in GPU memory (the result tensor of an operation).  The CipherText
// objects of the result tensor only hold a reference to it and their index: GMP integers are created on first
// access, the records are downloaded once for the whole block when somebody reads them.  This is what makes the
// reference's calling pattern -- Tensor<CipherText *> in and out of every op, every element a heap object the
// caller frees (benchmarks/local.cpp:99-117) -- cheap: a chain of operations never leaves the device.
struct DeviceBlock {
    std::shared_ptr<cofhe_hip_ctx> owner;     // keeps the GPU context alive as long as result elements exist
    cofhe_hip_ctx *ctx = nullptr;
    void *dptr = nullptr;
    size_t n_ct = 0;
    std::vector<uint32_t> host;          // records, downloaded on demand
    std::shared_ptr<std::atomic<uint64_t>> downloads;     // the cryptosystem's count of such downloads (block_downloads())
    std::once_flag fetched;
    std::mutex mat_mu;                   // serialises the lazy CipherText objects of THIS block (not of every block)
    DeviceBlock(std::shared_ptr<cofhe_hip_ctx> c, void *p, size_t n) : owner(std::move(c)), ctx(owner.get()), dptr(p), n_ct(n) {}
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { if (dptr) cofhe_hip_free(ctx, dptr); }
    // The records, downloaded once for the whole block.  A failure is LATCHED: the download error or the device status
    // word (a safety cap hit by the kernels that wrote these records: an operand was not a reduced form of this
    // discriminant) poisons the block, and every later records() -- another element, a retry, another thread -- throws the
    // same error again instead of handing out the downloaded garbage.  The status word itself is read WITHOUT clearing it:
    // it is per context, so every other block and thread that holds results of the faulty launch sees it too, until the
    // owner of the cryptosystem has dealt with it (HIPCryptoSystem::clear_device_status()).
    const uint32_t *records() {
        std::call_once(fetched, [this]() {              // never throws: an exception would leave the flag unset
            host.resize(n_ct * 2 * 168);
            if (downloads) downloads->fetch_add(1, std::memory_order_relaxed);
            if (cofhe_hip_download(ctx, host.data(), dptr, host.size() * 4, nullptr) != COFHE_HIP_OK) {
                poison = cofhe_hip_last_error();
                if (poison.empty()) poison = "cofhe_hip: download failed";
                return;
            }
            poison = device_status_message(ctx);
        });
        if (!poison.empty()) throw std::runtime_error(poison);
        return host.data();
    }
    static std::string device_status_message(cofhe_hip_ctx *ctx) {
        uint32_t w = 0;
        if (cofhe_hip_device_status(ctx, &w, /*clear=*/0, nullptr) != COFHE_HIP_OK) {
            std::string e = cofhe_hip_last_error();
            return e.empty() ? std::string("cofhe_hip: status read failed") : e;
        }
        if (w == 0) return std::string();
        if (w == 32u)          // CF_ST_BAD_INDEX alone
            return "cofhe_hip: device status word 32 (an index gather met an index beyond its source and wrote the fill record; results discarded)";
        return "cofhe_hip: device status word " + std::to_string(w) +
               " (a loop cap was hit: an operand was not a reduced form of this discriminant; results discarded)" +
               (w & 32u ? "; bit 32: an index gather met an index beyond its source" : "");
    }
    static void throw_on_device_status(cofhe_hip_ctx *ctx) {
        const std::string m = device_status_message(ctx);
        if (!m.empty()) throw std::runtime_error(m);
    }
    std::string poison;                  // written once inside call_once, read after it
};

class CipherText {
  public:
    CipherText() = default;
    CipherText(QFI c1, QFI c2) : c1_(std::move(c1)), c2_(std::move(c2)), have_(true) {}
    // element `index` of a device-resident result block
    CipherText(std::shared_ptr<DeviceBlock> blk, size_t index) : blk_(std::move(blk)), idx_(index), have_(false) {}
    // Copies are safe against a concurrent first read of the source (the reference's compute server shares result
    // tensors between its 8 threads): a source whose values exist is copied with them, one that is still lazy -- or
    // being materialised right now -- is copied as the (immutable) block reference and index only.
    CipherText(const CipherText &o) : blk_(o.blk_), idx_(o.idx_), have_(false) { take_values(o); }
    CipherText &operator=(const CipherText &o) {
        if (this != &o) {
            blk_ = o.blk_;
            idx_ = o.idx_;
            have_.store(false, std::memory_order_relaxed);
            dirty_.store(false, std::memory_order_relaxed);
            take_values(o);
        }
        return *this;
    }
    const QFI &c1() const { materialise(); return c1_; }
    const QFI &c2() const { materialise(); return c2_; }
    // writable components (the reference accumulates in place: cl_g.nucomp(res->c1(), res->c1(), x->c1()),
    // include/smpc/ciphertext_multiplications.hpp:97-98).  Tensor elements are non-const pointers, so plain READS written as
    // in the reference (cts.at(i)->c1(), cpu_cryptosystem_tensor_ops.inl:175) select these overloads too -- from several
    // server threads at once on a shared result tensor.  They therefore change nothing but an atomic flag: the values are
    // materialised (under the block's lock), the object is marked host-dirty -- its values may now differ from the
    // block's records -- and block() stops offering the device copy.  blk_ / idx_ themselves are never written here.
    QFI &c1() { touch(); return c1_; }
    QFI &c2() { touch(); return c2_; }
    // device backing, if any and still valid (HIPCryptoSystem uses it to keep chains on the GPU)
    const std::shared_ptr<DeviceBlock> &block() const {
        static const std::shared_ptr<DeviceBlock> none;
        return dirty_.load(std::memory_order_acquire) ? none : blk_;
    }
    size_t block_index() const { return idx_; }

  private:
    static QFI form_of(const uint32_t *rec) {
        Mpz a, b, c;
        mpz_import(a.get(), 40, -1, 4, 0, 0, rec + 0);
        mpz_import(b.get(), 40, -1, 4, 0, 0, rec + 40);
        mpz_import(c.get(), 80, -1, 4, 0, 0, rec + 80);
        if (rec[160]) b.neg();
        return QFI(std::move(a), std::move(b), std::move(c));
    }
    void take_values(const CipherText &o) {
        // a host-dirty source is being (or has been) written through c1() / c2(): its owner must not do that while somebody
        // copies it (as with any value type); the copy takes the values as they are and is host-dirty itself
        if (o.dirty_.load(std::memory_order_acquire)) dirty_.store(true, std::memory_order_release);
        if (o.have_.load(std::memory_order_acquire)) {
            c1_ = o.c1_;
            c2_ = o.c2_;
            have_.store(true, std::memory_order_release);
        } else if (!blk_) {
            have_.store(true, std::memory_order_release);       // default-constructed source: empty forms
        }
    }
    void materialise() const {
        if (have_.load(std::memory_order_acquire)) return;
        std::lock_guard<std::mutex> lk(blk_->mat_mu);
        if (have_.load(std::memory_order_relaxed)) return;
        const uint32_t *r = blk_->records() + idx_ * 2 * 168;
        c1_ = form_of(r);
        c2_ = form_of(r + 168);
        have_.store(true, std::memory_order_release);
    }
    void touch() {
        materialise();
        dirty_.store(true, std::memory_order_release);
    }
    mutable QFI c1_, c2_;
    std::shared_ptr<DeviceBlock> blk_;
    size_t idx_ = 0;
    mutable std::atomic<bool> have_{true};
    std::atomic<bool> dirty_{false};       // values handed out writable: the device records no longer stand for this object
};

enum class Precision { FP32, FP64 };
// Randomness of the tensor operations.  None (the default): encrypt_tensor draws ONE r per call, as the reference does
// (tensor_ops.inl:1-19), and the tensor operations are deterministic.  PerElement: every ciphertext that encrypt_tensor,
// add_ciphertext_tensors, scal_ciphertext_tensors or negate_ciphertext_tensor returns carries its own fresh r -- the
// reference's compiled-out ADD_RANDOMNESS_IN_HOMOMORPHIC_OPERATIONS + DIFFERENT_RANDOMNESS_FOR_EACH_OPERATION mode
// (cpu_cryptosystem_vector_ops.inl:1-2).  With one r per tensor, c2_i o c2_j^-1 = f^(m_i - m_j) leaks every plaintext difference.
enum class TensorRandomness { None, PerElement };
enum class SecurityLevel { LOW, MEDIUM, HIGH };

// ---- the engine -----------------------------------------------------------------------------
class HIPCryptoSystem {
  public:
    using SecretKey = Mpz;
    using PublicKey = QFI;
    using PlainText = Mpz;
    using CipherText = CoFHE::CipherText;
    using PartDecryptionResult = QFI;
    using SecretKeyShare = Mpz;

    // device-resident ciphertext tensor (extension: keeps a chain of ops in HBM)
    class DeviceTensor {
      public:
        DeviceTensor() = default;
        DeviceTensor(const DeviceTensor &) = delete;
        DeviceTensor &operator=(const DeviceTensor &) = delete;
        DeviceTensor(DeviceTensor &&o) noexcept { *this = std::move(o); }
        DeviceTensor &operator=(DeviceTensor &&o) noexcept {
            release();
            ctx_ = o.ctx_; ptr_ = o.ptr_; shape_ = std::move(o.shape_); n_ = o.n_; keep_ = std::move(o.keep_);
            o.ptr_ = nullptr; o.n_ = 0;
            return *this;
        }
        ~DeviceTensor() { release(); }
        const std::vector<size_t> &shape() const { return shape_; }
        size_t num_elements() const { return n_; }
        void *data() const { return ptr_; }

      private:
        friend class HIPCryptoSystem;
        void release() {
            if (ptr_ && !keep_) cofhe_hip_free(ctx_, ptr_);      // a view of a DeviceBlock does not own the memory
            ptr_ = nullptr;
            keep_.reset();
        }
        cofhe_hip_ctx *ctx_ = nullptr;
        void *ptr_ = nullptr;
        std::shared_ptr<DeviceBlock> keep_;     // set when this tensor is a view of a result block
        std::vector<size_t> shape_;
        size_t n_ = 0;     // ciphertexts
    };

    // Fresh parameters (literature restatement of CL_HSM2k setup; see DESIGN.md "unpinned").
    HIPCryptoSystem(uint32_t security_level, uint32_t k, int device = 0, uint64_t seed = std::random_device{}())
        : sec_level_(security_level), k_(k), device_(device) {
        gmp_randinit_mt(rng_);
        gmp_randseed_ui(rng_, seed);
        generate_parameters();
        open_device();
        compute_generator();
        pack_generators();
        init_mpf();
    }
    // Existing parameters: N (odd, as generated above) and the generator h of the system.
    HIPCryptoSystem(uint32_t security_level, uint32_t k, const Mpz &N, const QFI &h, int device = 0,
                    uint64_t seed = std::random_device{}())
        : sec_level_(security_level), k_(k), device_(device), N_(N), h_(h) {
        gmp_randinit_mt(rng_);
        gmp_randseed_ui(rng_, seed);
        derive_from_N();
        open_device();
        pack_generators();
        init_mpf();
    }
    HIPCryptoSystem(const HIPCryptoSystem &o)
        : sec_level_(o.sec_level_), k_(o.k_), device_(o.device_), N_(o.N_), deltaK_(o.deltaK_), delta_(o.delta_),
          f_(o.f_), h_(o.h_), f_rec_(o.f_rec_), h_rec_(o.h_rec_), exponent_bound_(o.exponent_bound_), rerandomize_(o.rerandomize_),
          resident_gather_(o.resident_gather_), tensor_randomness_(o.tensor_randomness_) {
        gmp_randinit_mt(rng_);
        gmp_randseed_ui(rng_, std::random_device{}());     // a copy draws fresh randomness (hpp:37-40)
        open_device();
        init_mpf();
    }
    HIPCryptoSystem &operator=(const HIPCryptoSystem &) = delete;
    ~HIPCryptoSystem() {
        ctx_owner_.reset();                 // the context itself goes when the last result block has gone
        gmp_randclear(rng_);
        mpf_clear(scaling_factor_); mpf_clear(mM_); mpf_clear(mM_half_);
    }

    const Mpz &discriminant() const { return delta_; }
    const QFI &generator_h() const { return h_; }
    const QFI &generator_f() const { return f_; }
    const Mpz &modulus_N() const { return N_; }
    cofhe_hip_ctx *context() const { return ctx_; }

    // ---- keys --------------------------------------------------------------------------------
    SecretKey keygen() const {
        Mpz sk;
        std::lock_guard<std::mutex> lk(rng_mutex_);
        mpz_urandomm(sk.get(), rng_, exponent_bound_.get());
        return sk;
    }
    PublicKey keygen(const SecretKey &sk) const { return pow_fixed_base(h_, sk); }

    // ---- plaintext encoding: the reference's own GMP calls (cpu_cryptosystem.inl:49-87) ------
    PlainText make_plaintext(float value) const {
        mpf_t x;
        mpf_init(x);
        mpf_set_d(x, value);
        mpf_mul(x, x, scaling_factor_);
        if (value < 0) mpf_add(x, x, mM_);
        Mpz r;
        mpz_set_f(r.get(), x);
        mpf_clear(x);
        return r;
    }
    float get_float_from_plaintext(const PlainText &pt) const {
        mpf_t num;
        mpf_init(num);
        mpf_set_z(num, pt.get());
        if (mpf_cmp(num, mM_half_) >= 0) mpf_sub(num, num, mM_);
        mpf_div(num, num, scaling_factor_);
        float r = (float)mpf_get_d(num);
        mpf_clear(num);
        return r;
    }

    uint32_t message_bits() const { return k_; }
    // uniform plaintext below 2^bits (Beaver triplets, smpc_local.hpp)
    PlainText random_plaintext(uint32_t bits) const {
        Mpz r;
        std::lock_guard<std::mutex> lk(rng_mutex_);
        mpz_urandomb(r.get(), rng_, bits);
        return r;
    }
    // ---- plaintext arithmetic (integers, no reduction: cpu_cryptosystem.inl:100-112) ------------
    PlainText add_plaintexts(const PlainText &a, const PlainText &b) const {
        Mpz r;
        mpz_add(r.get(), a.get(), b.get());
        return r;
    }
    PlainText multiply_plaintexts(const PlainText &a, const PlainText &b) const {
        Mpz r;
        mpz_mul(r.get(), a.get(), b.get());
        return r;
    }
    PlainText negate_plaintext(const PlainText &s) const { return make_plaintext(-get_float_from_plaintext(s)); }
    // element-wise, any shape (reference: tensor_ops.inl:123-133)
    Tensor<PlainText *> negate_plaintext_tensor(const Tensor<PlainText *> &s) const {
        if (s.is_zero_degree()) return Tensor<PlainText *>(new PlainText(negate_plaintext(*s.get_value())));
        Tensor<PlainText *> res(s.shape(), nullptr);
        res.flatten();
        Tensor<PlainText *> flat = s;
        flat.flatten();
        for (size_t i = 0; i < s.num_elements(); i++) res[i] = new PlainText(negate_plaintext(*flat[i]));
        res.reshape(s.shape());
        return res;
    }
    // uniform below the cleartext bound 2^k (reference: cpu_cryptosystem.inl:31-34, rand_gen.random_mpz(cleartext_bound))
    PlainText generate_random_plaintext() const {
        Mpz bound, r;
        mpz_setbit(bound.get(), k_);
        std::lock_guard<std::mutex> lk(rng_mutex_);
        mpz_urandomm(r.get(), rng_, bound.get());
        return r;
    }
    // (a, b, a b) with a, b uniform below 10 -- the reference's own bound (cpu_cryptosystem.inl:36-47: "can cause overflow
    // if the k is less than 20"); consumed by BeaversTripletGenerator (include/smpc/beavers_triplet_generation.hpp:23)
    Vector<PlainText> generate_random_beavers_triplet() const {
        Vector<PlainText> res;
        Mpz bound(10ul), a, b;
        {
            std::lock_guard<std::mutex> lk(rng_mutex_);
            mpz_urandomm(a.get(), rng_, bound.get());
            mpz_urandomm(b.get(), rng_, bound.get());
        }
        res.push_back(a);
        res.push_back(b);
        res.push_back(multiply_plaintexts(res[0], res[1]));
        return res;
    }
    // 0-D and 1-D only, like the reference (tensor_ops.inl:75-121)
    Tensor<PlainText *> add_plaintext_tensors(const Tensor<PlainText *> &a, const Tensor<PlainText *> &b) const {
        return plaintext_tensor_op(a, b, false);
    }
    Tensor<PlainText *> multiply_plaintext_tensors(const Tensor<PlainText *> &a, const Tensor<PlainText *> &b) const {
        return plaintext_tensor_op(a, b, true);
    }

    // ---- encryption (GPU: c1 = h^r, c2 = f^m o pk^r; one r per tensor, tensor_ops.inl:7-15) --
    CipherText encrypt(const PublicKey &pk, const PlainText &pt) const {
        return single(encrypt_tensor(pk, Tensor<PlainText *>(1, const_cast<PlainText *>(&pt))));
    }
    Tensor<CipherText *> encrypt_tensor(const PublicKey &pk, const Tensor<PlainText *> &pts) const {
        if (tensor_randomness_ == TensorRandomness::PerElement) return encrypt_tensor_fresh(pk, pts);
        Mpz r;
        {
            std::lock_guard<std::mutex> lk(rng_mutex_);      // the object is shared between server threads
            mpz_urandomm(r.get(), rng_, exponent_bound_.get());
        }
        // c1 = h^r and pk^r once per tensor (two ladders), then one fixed-base kernel for all f^(m_i) o pk^r
        const size_t E = pts.num_elements();
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        std::vector<uint32_t> base(h_rec_.begin(), h_rec_.end()), ex(2 * EXPW, 0);
        base.insert(base.end(), pkrec.begin(), pkrec.end());
        pack_exponent(r, &ex[0]);
        pack_exponent(r, &ex[EXPW]);
        Staged plain = stage(pack_exponents(pts)), hp = device_buffer(base.size() * 4);
        // h^r and pk^r: fixed bases -> product trees over the cached tables h^(2^j), pk^(2^j); both operands are host records
        check(cofhe_hip_pow_fixed_base_records(ctx_, 2, base.data(), ex.data(), hp.ptr, nullptr));
        DeviceTensor out = alloc(shape_of(pts), E);
        check(cofhe_hip_encrypt_records(ctx_, plain.ptr, hp.ptr, f_rec_.data(), out.ptr_, E, k_, nullptr));
        return download(std::move(out));
    }
    // decryption, all on the GPU: c2 o (c1^sk)^-1 = f^m, m read off bit by bit from the 2-adic
    // valuation visible in the reduced form (kernel k_decrypt; DESIGN.md, "unpinned")
    PlainText decrypt(const SecretKey &sk, const CipherText &ct) const {
        return single(decrypt_tensor(sk, Tensor<CipherText *>(1, const_cast<CipherText *>(&ct))));
    }
    Tensor<PlainText *> decrypt_tensor(const SecretKey &sk, const Tensor<CipherText *> &cts) const {
        const size_t E = cts.num_elements(), ow = (k_ + 31) / 32 + 1;
        DeviceTensor dc = upload(cts);
        Staged dsk = stage(exponent_record(sk)), dout = device_buffer(E * ow * 4);
        check(cofhe_hip_decrypt_records(ctx_, dc.ptr_, dsk.ptr, f_rec_.data(), dout.ptr, E, k_, nullptr));
        return read_plaintexts(dout.ptr, E, ow, shape_of(cts), false, "ciphertext does not decrypt into <f>");
    }

    // ---- threshold decryption (reference: cpu_cryptosystem_distributed.inl, tensor_ops.inl:35-73) ---
    // keygen(sk, t, n): linear integer secret sharing with the AND/OR distribution matrix of
    // cpu_cryptosystem_distributed.inl:22-158; result[party] = that party's shares, one per
    // threshold set containing it, in lexicographic order of the sets (:287-309).
    Vector<Vector<SecretKeyShare>> keygen(const SecretKey &sk, size_t threshold, size_t num_parties) const {
        std::vector<std::vector<int>> M = distribution_matrix(num_parties, threshold);
        const size_t cols = M[0].size();
        std::vector<Mpz> rho(cols);
        rho[0] = sk;
        {
            std::lock_guard<std::mutex> lk(rng_mutex_);
            for (size_t j = 1; j < cols; j++) mpz_urandomm(rho[j].get(), rng_, exponent_bound_.get());
        }
        std::vector<Mpz> rows(M.size());
        for (size_t i = 0; i < M.size(); i++)
            for (size_t j = 0; j < cols; j++) {
                if (M[i][j] > 0) mpz_addmul_ui(rows[i].get(), rho[j], (unsigned long)M[i][j]);
                else if (M[i][j] < 0) mpz_submul_ui(rows[i].get(), rho[j], (unsigned long)(-M[i][j]));
            }
        Vector<Vector<SecretKeyShare>> shares(num_parties);
        std::vector<size_t> comb(threshold);
        for (size_t i = 0; i < threshold; i++) comb[i] = i;
        for (size_t i = 0; i * threshold < M.size(); i++) {
            for (size_t j = 0; j < threshold; j++) shares[comb[j]].push_back(rows[i * threshold + j]);
            long j = (long)threshold - 1;                          // next lexicographic t-subset
            while (j >= 0 && comb[j] == num_parties - threshold + j) j--;
            if (j >= 0) {
                comb[j]++;
                for (size_t q = j + 1; q < threshold; q++) comb[q] = comb[j] + q - j;
            }
        }
        return shares;
    }
    // d_i = c1^share for every element: one GPU power ladder per ciphertext (kernel k_pow, stride 2)
    PartDecryptionResult part_decrypt(const SecretKeyShare &sks, const CipherText &ct) const {
        return single(part_decrypt_tensor(sks, Tensor<CipherText *>(1, const_cast<CipherText *>(&ct))));
    }
    Tensor<PartDecryptionResult *> part_decrypt_tensor(const SecretKeyShare &sks, const Tensor<CipherText *> &cts) const {
        const size_t E = cts.num_elements();
        DeviceTensor dc = upload(cts);
        Staged dsh = stage(exponent_record(sks)), dout = device_buffer(E * REC * 4);
        check(cofhe_hip_part_decrypt_records(ctx_, dc.ptr_, dsh.ptr, dout.ptr, E, nullptr));
        std::vector<QFI> d = read_forms(dout.ptr, E);
        Tensor<PartDecryptionResult *> out(shape_of(cts), nullptr);
        for (size_t i = 0; i < E; i++) out[i] = new PartDecryptionResult(std::move(d[i]));
        return out;
    }
    // m = dlog_f(c2 o (d_0 o d_1^-1 o ... o d_(t-1)^-1)^-1), lambda = (1, -1, ..., -1)
    // (compute_lambda / compute_d / finalDecrypt, cpu_cryptosystem_distributed.inl:215-285)
    PlainText combine_part_decryption_results(const CipherText &ct, const Vector<PartDecryptionResult> &pdrs) const {
        Tensor<CipherText *> t(1, const_cast<CipherText *>(&ct));
        Vector<Tensor<PartDecryptionResult *>> ps;
        for (const auto &p : pdrs) ps.push_back(Tensor<PartDecryptionResult *>(1, const_cast<PartDecryptionResult *>(&p)));
        return single(combine_part_decryption_results_tensor(t, ps));
    }
    Tensor<PlainText *> combine_part_decryption_results_tensor(const Tensor<CipherText *> &cts,
                                                               const Vector<Tensor<PartDecryptionResult *>> &pdrs) const {
        const size_t E = cts.num_elements(), T = pdrs.size();
        if (T == 0) throw std::invalid_argument("no partial decryptions");
        DeviceTensor dc = upload(cts);
        std::vector<uint32_t> recs(T * E * REC, 0);
        for (size_t j = 0; j < T; j++) {
            if (pdrs[j].num_elements() != E) throw std::invalid_argument("Tensor shapes must be equal");
            Tensor<PartDecryptionResult *> flat = pdrs[j];
            flat.flatten();
            pack_forms(E, &recs[j * E * REC], [&](size_t i) -> const QFI & { return *flat[i]; });
        }
        std::vector<int32_t> lambda(T, -1);
        lambda[0] = 1;
        const size_t ow = (k_ + 31) / 32 + 1;
        Staged dp = stage(std::move(recs)), dout = device_buffer(E * ow * 4);
        check(cofhe_hip_combine_part_decryptions_records(ctx_, dc.ptr_, dp.ptr, (uint32_t)T, lambda.data(), f_rec_.data(), dout.ptr,
                                                         E, k_, nullptr));
        return read_plaintexts(dout.ptr, E, ow, shape_of(pdrs[0]), false, "partial decryptions do not combine into <f>");
    }
    // binary format of a partial-decryption tensor (cpu_cryptosystem.inl:510-635)
    String serialize_part_decryption_result_tensor(const Tensor<PartDecryptionResult *> &t) const {
        const size_t E = t.num_elements();
        std::vector<uint32_t> recs(E * REC, 0);
        Tensor<PartDecryptionResult *> flat = t;
        flat.flatten();
        pack_forms(E, recs.data(), [&](size_t i) -> const QFI & { return *flat[i]; });
        std::vector<uint32_t> shape(t.shape().begin(), t.shape().end());
        uint8_t *bytes = nullptr;
        size_t len = 0;
        check(cofhe_hip_pdr_records_to_bytes(recs.data(), E, (uint32_t)shape.size(), shape.data(), &bytes, &len));
        String s((const char *)bytes, len);
        cofhe_hip_host_free(bytes);
        return s;
    }
    Tensor<PartDecryptionResult *> deserialize_part_decryption_result_tensor(const String &data) const {
        uint32_t ndim = 0, shape[8];
        uint32_t *recs = nullptr;
        uint64_t n = 0;
        check(cofhe_hip_pdr_bytes_to_records((const uint8_t *)data.data(), data.size(), &ndim, shape, &recs, &n));
        std::vector<size_t> sh(shape, shape + ndim);
        Tensor<PartDecryptionResult *> out(sh, nullptr);
        Tensor<PartDecryptionResult *> flat = out;
        flat.flatten();
        COFHE_HOST_PARALLEL_FOR
        for (uint64_t i = 0; i < n; i++) flat[i] = new PartDecryptionResult(unpack_form(recs + i * REC));
        cofhe_hip_host_free(recs);
        return out;
    }

    // ---- the hot path ------------------------------------------------------------------------
    // element-wise homomorphic addition (reference: tensor_ops.inl:197-267; pk unused there too)
    Tensor<CipherText *> add_ciphertext_tensors(const PublicKey &pk, const Tensor<CipherText *> &ct1,
                                                const Tensor<CipherText *> &ct2) const {
        (void)pk;
        if (ct1.is_zero_degree() && ct2.is_zero_degree()) {
            return Tensor<CipherText *>(new CipherText(add_ciphertexts(pk, *ct1.get_value(), *ct2.get_value())));
        }
        if (ct1.is_zero_degree() != ct2.is_zero_degree() || ct1.shape() != ct2.shape())
            throw std::invalid_argument("Tensor shapes must be equal");
        DeviceTensor a = upload(ct1), b = upload(ct2);
        DeviceTensor r = add_ciphertext_tensors(a, b);
        rerandomize_result(pk, r);
        return download(std::move(r));
    }
    // Scalar forms.  The reference re-randomises their result with a fresh r (hsm2k.add_ciphertexts / scal_ciphertexts
    // take rand_gen: cpu_cryptosystem.inl:21-29, reached by the 0-D tensor branches tensor_ops.inl:199-202, 275-278):
    // (c1 h^r, c2 pk^r).  Same here by default; set_rerandomize(false) gives the bare composition / power, which is
    // what a byte-for-byte parity check needs (the tensor forms the reference benchmarks are deterministic anyway).
    void set_rerandomize(bool on) { rerandomize_ = on; }
    // TensorRandomness::PerElement: fresh r per ciphertext for encrypt_tensor and the outputs of the tensor operations
    void set_tensor_randomness(TensorRandomness mode) { tensor_randomness_ = mode; }
    TensorRandomness tensor_randomness() const { return tensor_randomness_; }
    // (c1_i o h^r_i, c2_i o pk^r_i) with a fresh r_i < exponent_bound per element: what a tensor needs before it leaves the
    // process, whatever the mode (one batched comb call, cofhe_hip_rerandomize_records)
    Tensor<CipherText *> rerandomize_ciphertext_tensor(const PublicKey &pk, const Tensor<CipherText *> &cts) const {
        if (cts.is_zero_degree()) {
            Tensor<CipherText *> r = rerandomize_ciphertext_tensor(pk, Tensor<CipherText *>(1, cts.get_value()));
            return Tensor<CipherText *>(r.at(0));
        }
        DeviceTensor in = upload(cts);
        DeviceTensor out = alloc(cts.shape(), cts.num_elements());
        rerandomize_into(pk, in, out);
        return download(std::move(out));
    }
    // The device status word is sticky: once a kernel has hit a safety cap (an operand that was not a reduced form of this
    // discriminant), every read of results of this cryptosystem throws until its owner acknowledges the fault here.
    // Returns the word that was set.
    uint32_t clear_device_status() const {
        uint32_t w = 0;
        check(cofhe_hip_device_status(ctx_, &w, /*clear=*/1, nullptr));
        return w;
    }
    bool rerandomize() const { return rerandomize_; }
    CipherText add_ciphertexts(const PublicKey &pk, const CipherText &ct1, const CipherText &ct2) const {
        std::vector<QFI> r = compose_forms({ct1.c1(), ct1.c2()}, {ct2.c1(), ct2.c2()});
        return rerandomized(pk, CipherText(r[0], r[1]));
    }
    CipherText scal_ciphertext(const PublicKey &pk, const PlainText &s, const CipherText &ct) const {
        std::vector<QFI> r = pow_forms({ct.c1(), ct.c2()}, {s, s});
        return rerandomized(pk, CipherText(r[0], r[1]));
    }

    // plaintext (x) ciphertext: 0-D, 1-D x 1-D element-wise, 2-D x 2-D matrix product
    // (reference: tensor_ops.inl:269-462).  The 2-D branch starts every output from a fresh
    // encryption of zero (tensor_ops.inl:352); pass `zero` to make the call reproducible.
    Tensor<CipherText *> scal_ciphertext_tensors(const PublicKey &pk, const Tensor<PlainText *> &s,
                                                 const Tensor<CipherText *> &cts, const CipherText *zero = nullptr) const {
        if (s.ndim() > 2 || cts.ndim() > 2) throw std::invalid_argument("Tensors must be 0D, 1D or 2D for now");
        if (s.is_zero_degree() && cts.is_zero_degree())
            return Tensor<CipherText *>(new CipherText(scal_ciphertext(pk, *s.get_value(), *cts.get_value())));
        std::vector<uint32_t> ex = pack_exponents(s);
        DeviceTensor dc = upload(cts);
        Staged dex = stage(std::move(ex));
        if (s.is_column_vector() && cts.is_column_vector()) {
            if (s.shape()[0] != cts.shape()[0]) throw std::invalid_argument("Vector sizes must be equal");
            DeviceTensor out = alloc(cts.shape(), cts.num_elements());
            check(cofhe_hip_pow_records(ctx_, dc.ptr_, dex.ptr, out.ptr_, cts.num_elements(), nullptr));
            rerandomize_result(pk, out);
            return download(std::move(out));
        }
        if (s.ndim() != 2 || cts.ndim() != 2) throw std::invalid_argument("Tensors must be 0D, 1D or 2D for now");
        const size_t n = cts.shape()[0], m = cts.shape()[1], p = s.shape()[1];
        // DELIBERATE DEVIATION: the reference checks nothing here and, with s.shape[0] != cts.shape[1],
        // reads rows of the plaintext tensor that do not exist (tensor_ops.inl:396-402: s_vec + j * p for j < cts.shape[1]).
        // There is no faithful result to reproduce, so the call is refused -- with a message of its own, not add's.
        if (s.shape()[0] != m)
            throw std::invalid_argument("scal_ciphertext_tensors: inner dimensions differ (plaintext rows != ciphertext columns)");
        DeviceTensor dz = zero_tensor(pk, zero);
        DeviceTensor out = alloc({n, p}, n * p);
        check(cofhe_hip_scal_matmul_records(ctx_, dc.ptr_, dex.ptr, dz.ptr_, out.ptr_, (uint32_t)n, (uint32_t)m, (uint32_t)p,
                                            nullptr));
        rerandomize_result(pk, out);           // one fresh r per output (the reference's branch reuses one per row)
        return download(std::move(out));
    }

    // plaintext matrix (n x m) . ciphertext matrix (m x p): res[i,k] = zero o prod_j cts[j,k]^s[i,j], a linear layer y = W x
    // with plaintext weights.  The reference has no such operation (its 2-D scal_ciphertext_tensors has the ciphertext
    // matrix on the left); the engine runs that product on transposed views (cofhe_hip_matmul_plain_ct_records).  Starts
    // from a fresh encryption of zero like the 2-D branch above; pass `zero` to make the call reproducible.
    Tensor<CipherText *> matmul_plaintext_ciphertext_tensors(const PublicKey &pk, const Tensor<PlainText *> &s,
                                                             const Tensor<CipherText *> &cts, const CipherText *zero = nullptr) const {
        if (s.ndim() != 2 || cts.ndim() != 2) throw std::invalid_argument("matmul_plaintext_ciphertext_tensors: both operands must be 2D");
        DeviceTensor out = matmul_plaintext_ciphertext_tensors(s, upload(cts), zero_tensor(pk, zero));
        rerandomize_result(pk, out);           // one fresh r per output, as scal_ciphertext_tensors
        return download(std::move(out));
    }
    // the same on resident operands; deterministic (no re-randomisation), like the other DeviceTensor members
    DeviceTensor matmul_plaintext_ciphertext_tensors(const Tensor<PlainText *> &s, const DeviceTensor &cts, const DeviceTensor &zero) const {
        if (s.ndim() != 2 || cts.shape_.size() != 2) throw std::invalid_argument("matmul_plaintext_ciphertext_tensors: both operands must be 2D");
        const size_t n = s.shape()[0], m = s.shape()[1], p = cts.shape_[1];
        if (cts.shape_[0] != m)
            throw std::invalid_argument("matmul_plaintext_ciphertext_tensors: inner dimensions differ (plaintext columns != ciphertext rows)");
        if (zero.n_ != 1) throw std::invalid_argument("matmul_plaintext_ciphertext_tensors: zero must be one ciphertext");
        Staged dex = stage(pack_exponents(s));
        DeviceTensor out = alloc({n, p}, n * p);
        check(cofhe_hip_matmul_plain_ct_records(ctx_, dex.ptr, cts.ptr_, zero.ptr_, out.ptr_, (uint32_t)n, (uint32_t)m, (uint32_t)p, nullptr));
        return out;
    }
    // 2-D convolution, channels last: plaintext filters w [kh, kw, C, Co] over the ciphertext image cts [B, H, W, C] with
    // strides and zero padding as {rows, columns}; res[b,oy,ox,co] = zero o prod cts[b, oy sh + dy - ph, ox sw + dx - pw, ci]^w[dy,dx,ci,co],
    // a tensor [B, Ho, Wo, Co] -- the next layer's input as it is.  The reference has no convolution; the engine builds no patch
    // matrix (cofhe_hip_conv2d_plain_ct_records).  A bias is add_plaintext_tensor on the result.  Starts from a fresh
    // encryption of zero like the 2-D scal_ciphertext_tensors; pass `zero` to make the call reproducible.
    Tensor<CipherText *> conv2d_plaintext_ciphertext_tensors(const PublicKey &pk, const Tensor<PlainText *> &w, const Tensor<CipherText *> &cts,
                                                             const std::array<size_t, 2> &stride = {1, 1}, const std::array<size_t, 2> &pad = {0, 0},
                                                             const CipherText *zero = nullptr) const {
        if (w.ndim() != 4 || cts.ndim() != 4) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: both operands must be 4D");
        if (w.shape()[2] != cts.shape()[3]) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: the channels of the filters and of the image differ");
        return conv2d_plaintext_ciphertext_tensors(pk, w, cts, stride, pad, {1, 1}, 1, zero);      // re-randomised there: one fresh r per output
    }
    // the same on resident operands; deterministic (no re-randomisation), like the other DeviceTensor members
    DeviceTensor conv2d_plaintext_ciphertext_tensors(const Tensor<PlainText *> &w, const DeviceTensor &cts, const DeviceTensor &zero,
                                                     const std::array<size_t, 2> &stride = {1, 1}, const std::array<size_t, 2> &pad = {0, 0}) const {
        if (w.ndim() != 4 || cts.shape_.size() != 4) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: both operands must be 4D");
        if (w.shape()[2] != cts.shape_[3]) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: the channels of the filters and of the image differ");
        if (zero.n_ != 1) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: zero must be one ciphertext");
        return conv2d_plaintext_ciphertext_tensors(w, cts, zero, stride, pad, {1, 1}, 1);      // the same launches (cofhe_hip.h)
    }
    // The same with dilation {rows, columns} and groups: filters w [kh, kw, C / groups, Co], output column co reads the channel
    // block of group co / (Co / groups) (cofhe_hip_conv2d_grouped_plain_ct_records).  groups = C = Co is a depthwise
    // convolution, 1 x 1 filters on top of that a per-channel scale.  Re-randomised like the overload above.
    Tensor<CipherText *> conv2d_plaintext_ciphertext_tensors(const PublicKey &pk, const Tensor<PlainText *> &w, const Tensor<CipherText *> &cts,
                                                             const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad,
                                                             const std::array<size_t, 2> &dilation, size_t groups, const CipherText *zero = nullptr) const {
        if (w.ndim() != 4 || cts.ndim() != 4) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: both operands must be 4D");
        DeviceTensor out = conv2d_plaintext_ciphertext_tensors(w, upload(cts), zero_tensor(pk, zero), stride, pad, dilation, groups);
        rerandomize_result(pk, out);
        return download(std::move(out));
    }
    DeviceTensor conv2d_plaintext_ciphertext_tensors(const Tensor<PlainText *> &w, const DeviceTensor &cts, const DeviceTensor &zero,
                                                     const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad,
                                                     const std::array<size_t, 2> &dilation, size_t groups) const {
        if (w.ndim() != 4 || cts.shape_.size() != 4) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: both operands must be 4D");
        if (groups == 0 || w.shape()[2] != cts.shape_[3] / groups)
            throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: the filters' channels are not those of a group of the image");
        if (zero.n_ != 1) throw std::invalid_argument("conv2d_plaintext_ciphertext_tensors: zero must be one ciphertext");
        const cofhe_hip_conv2d_geometry geo = conv_geometry({cts.shape_[0], cts.shape_[1], cts.shape_[2], cts.shape_[3], w.shape()[0], w.shape()[1],
                                                             w.shape()[3], stride[0], stride[1], pad[0], pad[1], dilation[0], dilation[1], groups});
        uint32_t Ho = 0, Wo = 0;
        check(cofhe_hip_conv2d_geometry_out_shape(&geo, &Ho, &Wo));
        Staged dex = stage(pack_exponents(w));
        DeviceTensor out = alloc({geo.B, Ho, Wo, geo.Co}, (size_t)geo.B * Ho * Wo * geo.Co);
        check(cofhe_hip_conv2d_grouped_plain_ct_records(ctx_, dex.ptr, cts.ptr_, zero.ptr_, out.ptr_, &geo, nullptr));
        return out;
    }
    // Sum pooling, channels last: res[b,oy,ox,c] = zero + sum over the kernel[0] x kernel[1] window at (oy stride[0] - pad[0],
    // ox stride[1] - pad[1]) of cts[b, ., ., c], a tensor [B, Ho, Wo, C] (cofhe_hip_sum_pool2d_records: the depthwise convolution
    // with filters of ones, kh kw - 1 additions per output).  Average pooling is this with 1 / (kh kw) folded into the next
    // layer's plaintext weights (that inverse does not exist mod 2^k for an even window), or the division by kh kw of
    // LocalCipherTextMultiplier::avg_pool2d_ciphertext_tensor (smpc_local.hpp).  Re-randomised like conv2d.
    Tensor<CipherText *> sum_pool2d_ciphertext_tensor(const PublicKey &pk, const Tensor<CipherText *> &cts, const std::array<size_t, 2> &kernel,
                                                      const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad = {0, 0},
                                                      const CipherText *zero = nullptr) const {
        if (cts.ndim() != 4) throw std::invalid_argument("sum_pool2d_ciphertext_tensor: the operand must be 4D");
        DeviceTensor out = sum_pool2d_ciphertext_tensor(upload(cts), zero_tensor(pk, zero), kernel, stride, pad);
        rerandomize_result(pk, out);
        return download(std::move(out));
    }
    // the same on resident operands; deterministic
    DeviceTensor sum_pool2d_ciphertext_tensor(const DeviceTensor &cts, const DeviceTensor &zero, const std::array<size_t, 2> &kernel,
                                              const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad = {0, 0}) const {
        if (cts.shape_.size() != 4) throw std::invalid_argument("sum_pool2d_ciphertext_tensor: the operand must be 4D");
        if (zero.n_ != 1) throw std::invalid_argument("sum_pool2d_ciphertext_tensor: zero must be one ciphertext");
        const size_t C = cts.shape_[3];
        const cofhe_hip_conv2d_geometry geo = conv_geometry({cts.shape_[0], cts.shape_[1], cts.shape_[2], C, kernel[0], kernel[1], C, stride[0], stride[1],
                                                             pad[0], pad[1], 1, 1, C ? C : 1});
        uint32_t Ho = 0, Wo = 0;
        check(cofhe_hip_conv2d_geometry_out_shape(&geo, &Ho, &Wo));
        DeviceTensor out = alloc({geo.B, Ho, Wo, geo.C}, (size_t)geo.B * Ho * Wo * geo.C);
        check(cofhe_hip_sum_pool2d_records(ctx_, cts.ptr_, zero.ptr_, out.ptr_, &geo, nullptr));
        return out;
    }
    // a (n x m) . b (m x p) mod 2^k on the device (k_plain_matmul): the E D term of a matrix Beaver triplet and the C = A B of
    // its generation.  The element-wise multiply_plaintext_tensors is a host loop and stays one.
    Tensor<PlainText *> matmul_plaintext_tensors(const Tensor<PlainText *> &a, const Tensor<PlainText *> &b) const {
        if (a.ndim() != 2 || b.ndim() != 2) throw std::invalid_argument("matmul_plaintext_tensors: both operands must be 2D");
        const size_t n = a.shape()[0], m = a.shape()[1], p = b.shape()[1];
        if (b.shape()[0] != m) throw std::invalid_argument("matmul_plaintext_tensors: inner dimensions differ");
        Staged da = stage(pack_exponents(a)), db = stage(pack_exponents(b)), dout = device_buffer(n * p * EXPW * 4);
        check(cofhe_hip_matmul_plain_plain_records(ctx_, da.ptr, db.ptr, dout.ptr, (uint32_t)n, (uint32_t)m, (uint32_t)p, k_, nullptr));
        return read_plaintexts(dout.ptr, n * p, EXPW, {n, p}, false);
    }
    // img [B, H, W, C] * w [kh, kw, C, Co] mod 2^k on the device (k_plain_conv2d), channels last, strides, zero padding and
    // dilation as {rows, columns}: a tensor [B, Ho, Wo, Co].  The E * D term of a convolution Beaver triplet and the
    // C = A * Bf of its generation; mirrors matmul_plaintext_tensors.
    Tensor<PlainText *> conv2d_plaintext_tensors(const Tensor<PlainText *> &img, const Tensor<PlainText *> &w, const std::array<size_t, 2> &stride = {1, 1},
                                                 const std::array<size_t, 2> &pad = {0, 0}, const std::array<size_t, 2> &dilation = {1, 1}) const {
        if (img.ndim() != 4 || w.ndim() != 4) throw std::invalid_argument("conv2d_plaintext_tensors: both operands must be 4D");
        if (w.shape()[2] != img.shape()[3]) throw std::invalid_argument("conv2d_plaintext_tensors: the channels of the filters and of the image differ");
        const cofhe_hip_conv2d_geometry geo = conv_geometry({img.shape()[0], img.shape()[1], img.shape()[2], img.shape()[3], w.shape()[0], w.shape()[1],
                                                             w.shape()[3], stride[0], stride[1], pad[0], pad[1], dilation[0], dilation[1], 1});
        uint32_t Ho = 0, Wo = 0;
        check(cofhe_hip_conv2d_geometry_out_shape(&geo, &Ho, &Wo));
        const size_t nout = (size_t)geo.B * Ho * Wo * geo.Co;
        Staged di = stage(pack_exponents(img)), dw = stage(pack_exponents(w)), dout = device_buffer(nout * EXPW * 4);
        check(cofhe_hip_conv2d_plain_plain_records(ctx_, di.ptr, dw.ptr, dout.ptr, &geo, k_, nullptr));
        return read_plaintexts(dout.ptr, nout, EXPW, {geo.B, Ho, Wo, geo.Co}, false);
    }
    // 2-D convolution with CIPHERTEXT filters, channels last: the plaintext image img [B, H, W, C] under the ciphertext filters
    // filters [kh, kw, C, Co]; res[b,oy,ox,co] = zero o prod filters[dy,dx,ci,co]^img[b, oy sh + dy dh - ph, ox sw + dx dw - pw, ci],
    // a tensor [B, Ho, Wo, Co] (cofhe_hip_conv2d_ct_filters_records: the patch matrix of the image is written once, transposed,
    // and a filter's table of odd powers serves every output position).  The E * [Bf] term of a convolution Beaver triplet
    // (LocalCipherTextMultiplier::conv2d_ciphertext_tensors).  Starts from a fresh encryption of zero and is re-randomised like
    // matmul_plaintext_ciphertext_tensors; pass `zero` to make the start reproducible.
    Tensor<CipherText *> conv2d_ciphertext_filters_tensors(const PublicKey &pk, const Tensor<PlainText *> &img, const Tensor<CipherText *> &filters,
                                                           const std::array<size_t, 2> &stride = {1, 1}, const std::array<size_t, 2> &pad = {0, 0},
                                                           const std::array<size_t, 2> &dilation = {1, 1}, const CipherText *zero = nullptr) const {
        if (img.ndim() != 4 || filters.ndim() != 4) throw std::invalid_argument("conv2d_ciphertext_filters_tensors: both operands must be 4D");
        DeviceTensor out = conv2d_ciphertext_filters_tensors(img, upload(filters), zero_tensor(pk, zero), stride, pad, dilation);
        rerandomize_result(pk, out);           // one fresh r per output
        return download(std::move(out));
    }
    // the same on resident operands; deterministic (no re-randomisation), like the other DeviceTensor members
    DeviceTensor conv2d_ciphertext_filters_tensors(const Tensor<PlainText *> &img, const DeviceTensor &filters, const DeviceTensor &zero,
                                                   const std::array<size_t, 2> &stride = {1, 1}, const std::array<size_t, 2> &pad = {0, 0},
                                                   const std::array<size_t, 2> &dilation = {1, 1}) const {
        if (img.ndim() != 4 || filters.shape_.size() != 4) throw std::invalid_argument("conv2d_ciphertext_filters_tensors: both operands must be 4D");
        if (filters.shape_[2] != img.shape()[3])
            throw std::invalid_argument("conv2d_ciphertext_filters_tensors: the channels of the filters and of the image differ");
        if (zero.n_ != 1) throw std::invalid_argument("conv2d_ciphertext_filters_tensors: zero must be one ciphertext");
        const cofhe_hip_conv2d_geometry geo = conv_geometry({img.shape()[0], img.shape()[1], img.shape()[2], img.shape()[3], filters.shape_[0],
                                                             filters.shape_[1], filters.shape_[3], stride[0], stride[1], pad[0], pad[1], dilation[0],
                                                             dilation[1], 1});
        uint32_t Ho = 0, Wo = 0;
        check(cofhe_hip_conv2d_geometry_out_shape(&geo, &Ho, &Wo));
        Staged dex = stage(pack_exponents(img));
        DeviceTensor out = alloc({geo.B, Ho, Wo, geo.Co}, (size_t)geo.B * Ho * Wo * geo.Co);
        check(cofhe_hip_conv2d_ct_filters_records(ctx_, dex.ptr, filters.ptr_, zero.ptr_, out.ptr_, &geo, nullptr));
        return out;
    }

    // res[i,k] = zero o prod_j x[i,j,k] for x of n*m*p ciphertexts (flat, row-major): the
    // accumulation loop of the ciphertext x ciphertext matrix product
    // (include/smpc/ciphertext_multiplications.hpp:85-101) as one kernel
    Tensor<CipherText *> accumulate_ciphertext_tensor(const CipherText &zero, const Tensor<CipherText *> &x, size_t n,
                                                      size_t m, size_t p) const {
        if (x.num_elements() != n * m * p) throw std::invalid_argument("Tensor shapes must be equal");
        DeviceTensor dx = upload(x);
        Tensor<CipherText *> zt(1, const_cast<CipherText *>(&zero));
        DeviceTensor dz = upload(zt);
        DeviceTensor out = alloc({n, p}, n * p);
        check(cofhe_hip_accumulate_records(ctx_, dx.ptr_, dz.ptr_, out.ptr_, (uint32_t)n, (uint32_t)m, (uint32_t)p, nullptr));
        return download(std::move(out));
    }

    CipherText negate_ciphertext(const PublicKey &pk, const CipherText &ct) const {
        return scal_ciphertext(pk, make_plaintext(-1), ct);
    }
    // ct -> ct^(2^k - 1): the reference raises both components to make_plaintext(-1) = 2^k - 1
    // (tensor_ops.inl:135-195), which is NOT the group inverse of c1 (h has odd order) -- the same
    // power is taken here; the signed-digit ladder of k_pow does it in k squarings + 1 composition.
    Tensor<CipherText *> negate_ciphertext_tensor(const PublicKey &pk, const Tensor<CipherText *> &ct) const {
        PlainText minus_one = make_plaintext(-1);
        Tensor<CipherText *> flat = ct;
        if (ct.is_zero_degree()) return Tensor<CipherText *>(new CipherText(scal_ciphertext(pk, minus_one, *ct.get_value())));
        flat.flatten();
        Tensor<PlainText *> s(flat.num_elements(), &minus_one);
        Tensor<CipherText *> r = scal_ciphertext_tensors(pk, s, flat);
        r.reshape(ct.shape());
        return r;
    }

    // ---- differences and plaintext addends without a negation or an encryption ----------------------------------------------
    // a - b element-wise: (a.c1 o b.c1^-1, a.c2 o b.c2^-1), one composition per record (the inverse of a reduced form is a
    // sign flip) where negate + add spends k + 2.  The compute node's SUBTRACT, which the reference answers "Not implemented"
    // (include/node/compute_request_handler.hpp:67-76, 342-344); shapes and ownership as add_ciphertext_tensors.
    Tensor<CipherText *> sub_ciphertext_tensors(const PublicKey &pk, const Tensor<CipherText *> &ct1,
                                                const Tensor<CipherText *> &ct2) const {
        if (ct1.is_zero_degree() && ct2.is_zero_degree())
            return Tensor<CipherText *>(new CipherText(sub_ciphertexts(pk, *ct1.get_value(), *ct2.get_value())));
        if (ct1.is_zero_degree() != ct2.is_zero_degree() || ct1.shape() != ct2.shape())
            throw std::invalid_argument("Tensor shapes must be equal");
        DeviceTensor a = upload(ct1), b = upload(ct2);
        DeviceTensor r = sub_ciphertext_tensors(a, b);
        rerandomize_result(pk, r);
        return download(std::move(r));
    }
    // scalar form, re-randomised under set_rerandomize as add_ciphertexts is
    CipherText sub_ciphertexts(const PublicKey &pk, const CipherText &ct1, const CipherText &ct2) const {
        Tensor<CipherText *> t1(1, const_cast<CipherText *>(&ct1)), t2(1, const_cast<CipherText *>(&ct2));
        DeviceTensor a = upload(t1), b = upload(t2);
        DeviceTensor d = sub_ciphertext_tensors(a, b);
        return rerandomized(pk, single(download(d)));              // eager copy: the element outlives the block
    }
    // (c1^-1, c2^-1): an encryption of -m mod 2^k at no composition.  Not the ciphertext negate_ciphertext_tensor returns
    // (ct^(2^k - 1), tensor_ops.inl:135-195, kept as it is); the plaintexts agree.  Deterministic in every mode.
    Tensor<CipherText *> invert_ciphertext_tensor(const Tensor<CipherText *> &ct) const {
        if (ct.is_zero_degree()) {
            Tensor<CipherText *> r = invert_ciphertext_tensor(Tensor<CipherText *>(1, ct.get_value()));
            return Tensor<CipherText *>(r.at(0));
        }
        DeviceTensor in = upload(ct);
        DeviceTensor out = alloc(ct.shape(), ct.num_elements());
        check(cofhe_hip_invert_records(ctx_, in.ptr_, out.ptr_, 2 * in.n_, nullptr));
        return download(std::move(out));
    }
    // ct + pt, ct - pt, pt - ct element-wise without encrypting pt: (c1, c2 o f^(+-pt)) against the cached table of f, where
    // the node's mixed ADD (compute_request_handler.hpp:384-403, 452-470) encrypts the plaintext -- h^r, pk^r, f^m -- and adds.
    // A tensor that shared its c1 still does afterwards.  In TensorRandomness::PerElement mode the same tree also carries a
    // fresh r per element: (c1 o h^r, c2 o pk^r o f^(+-pt)).
    Tensor<CipherText *> add_plaintext_tensor(const PublicKey &pk, const Tensor<CipherText *> &ct, const Tensor<PlainText *> &pt) const {
        return plaintext_addend(pk, ct, pt, 0);
    }
    Tensor<CipherText *> sub_plaintext_tensor(const PublicKey &pk, const Tensor<CipherText *> &ct, const Tensor<PlainText *> &pt) const {
        return plaintext_addend(pk, ct, pt, 1);
    }
    Tensor<CipherText *> plaintext_sub_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &pt, const Tensor<CipherText *> &ct) const {
        return plaintext_addend(pk, ct, pt, 2);
    }

    // ---- polynomials on ciphertext tensors from one opened value (cofhe_hip.h: power tuples) -----------------------------------
    // res[e] = prod_{i<d} bases[i][e]^exps[i][e]: d ciphertext tensors and d plaintext tensors of one shape, one ladder per record
    // whose squarings the d bases share (cofhe_hip_pow_dot_records), 1 <= d <= 8.  The reference has no such operation.
    Tensor<CipherText *> pow_dot_ciphertext_tensors(const PublicKey &pk, const Vector<Tensor<PlainText *>> &exps,
                                                    const Vector<Tensor<CipherText *>> &bases) const {
        const size_t d = bases.size();
        if (d == 0 || d > COFHE_HIP_POLY_MAX_DEGREE || exps.size() != d) throw std::invalid_argument("pow_dot_ciphertext_tensors: 1 to 8 bases, as many exponent tensors");
        const size_t E = bases[0].num_elements();
        std::vector<uint32_t> ex(d * E * EXPW, 0);
        for (size_t i = 0; i < d; i++) {
            if (exps[i].num_elements() != E) throw std::invalid_argument("Tensor shapes must be equal");
            pack_exponents(exps[i], ex.data() + i * E * EXPW);
        }
        DeviceTensor db = stack(bases);
        Staged dex = stage(std::move(ex));
        DeviceTensor out = alloc(shape_of(bases[0]), E);
        check(cofhe_hip_pow_dot_records(ctx_, db.ptr_, dex.ptr, out.ptr_, E, (uint32_t)d, nullptr));
        rerandomize_result(pk, out);
        return download(std::move(out));
    }
    // the Taylor shift of p = sum_j coef[j] X^j at every x[e] mod 2^k: d + 1 tensors of x's shape, res[i][e] = q_i(x[e]) =
    // sum_{j>=i} C(j,i) coef[j] x[e]^(j-i) (cofhe_hip_poly_shift_records); res[0] is p(x)
    Vector<Tensor<PlainText *>> poly_shift_plaintext_tensor(const Tensor<PlainText *> &coef, const Tensor<PlainText *> &x) const {
        const size_t d1 = coef.num_elements(), E = x.num_elements();
        if (d1 == 0 || d1 > COFHE_HIP_POLY_MAX_DEGREE + 1) throw std::invalid_argument("poly_shift_plaintext_tensor: 1 to 9 coefficients");
        Staged dc = stage(pack_exponents(coef)), dx = stage(pack_exponents(x)), dq = device_buffer(d1 * E * EXPW * 4);
        check(cofhe_hip_poly_shift_records(ctx_, dc.ptr, dx.ptr, dq.ptr, E, (uint32_t)(d1 - 1), k_, nullptr));
        const Tensor<PlainText *> q = read_plaintexts(dq.ptr, d1 * E, EXPW, {d1 * E}, false);      // tensor-major: q_i of every element, i = 0..d
        Vector<Tensor<PlainText *>> res;
        for (size_t i = 0; i < d1; i++) {
            Tensor<PlainText *> t(shape_of(x), nullptr);
            for (size_t e = 0; e < E; e++) t[e] = q[i * E + e];
            res.push_back(t);
        }
        return res;
    }
    // the closing step of a polynomial evaluation: res[e] = (prod_{i=1..d} powers[i-1][e]^q_i(e[e])) o f^q_0(e[e]), an encryption
    // of p(x[e]) mod 2^k when powers[i-1][e] = [a_e^i] and e[e] = x[e] - a_e (cofhe_hip_poly_close_records: the shift, one
    // shared-squarings ladder per record and the plaintext addend, on the device from end to end).  coef: d + 1 coefficients,
    // pre-scaled by the caller so that every term carries one fixed-point scale.  Re-randomised in PerElement mode.
    Tensor<CipherText *> poly_close_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &coef, const Tensor<PlainText *> &e,
                                                      const Vector<Tensor<CipherText *>> &powers) const {
        const size_t d = powers.size(), E = e.num_elements();
        if (d == 0 || d > COFHE_HIP_POLY_MAX_DEGREE || coef.num_elements() != d + 1)
            throw std::invalid_argument("poly_close_ciphertext_tensor: d + 1 coefficients for d tensors of powers, 1 <= d <= 8");
        for (size_t i = 0; i < d; i++)
            if (powers[i].num_elements() != E) throw std::invalid_argument("Tensor shapes must be equal");
        std::vector<uint32_t> ec = pack_exponents(coef), ee = pack_exponents(e);
        DeviceTensor dp = stack(powers);
        Staged dc = stage(std::move(ec)), de = stage(std::move(ee));
        DeviceTensor out = alloc(shape_of(e), E);
        check(cofhe_hip_poly_close_records(ctx_, dc.ptr, de.ptr, dp.ptr_, f_rec_.data(), out.ptr_, E, (uint32_t)d, k_, nullptr));
        rerandomize_result(pk, out);
        return download(std::move(out));
    }
    // public divisors are host values: 1 <= D < 2^(k-1) for every one of them, and their count divides the element count n
    // (element e takes divisor e mod count: one divisor, one per channel of a channels-last tensor, or one per element)
    void check_divisors(const Tensor<PlainText *> &div, size_t n) const {
        const size_t nd = div.num_elements();
        if (nd == 0 || n % nd != 0) throw std::invalid_argument("divisors: their count must divide the element count");
        for (size_t i = 0; i < nd; i++)
            if (div[i]->sgn() <= 0 || div[i]->nbits() > k_ - 1) throw std::invalid_argument("divisors: 1 <= D < 2^(k-1)");
    }
    // res[e] = floor(s(v[e]) / div[e mod count]) mod 2^k, s the centred residue in [-2^(k-1), 2^(k-1)): the signed floor division
    // of cofhe_hip_divfloor_plain_records (k_plain_divfloor), of v's shape.  Both halves of a division pair and the quotient
    // of an opened value come from here.
    Tensor<PlainText *> divide_plaintext_tensor(const Tensor<PlainText *> &v, const Tensor<PlainText *> &div) const {
        const size_t E = v.num_elements(), nd = div.num_elements();
        check_divisors(div, E);
        Staged dv = stage(pack_exponents(v)), dd = stage(pack_exponents(div)), dq = device_buffer(E * EXPW * 4);
        check(cofhe_hip_divfloor_plain_records(ctx_, dv.ptr, dd.ptr, nd, dq.ptr, E, k_, nullptr));
        return read_plaintexts(dq.ptr, E, EXPW, shape_of(v), false);
    }
    // the closing step of a division by public divisors: res[e] = (c1, c2 o f^(e_q)) of rq[e], e_q = floor(s(e[e]) / div[e mod
    // count]) mod 2^k -- an encryption of floor(s(x[e]) / D) or one less when rq[e] = [r_q] of the element's division pair and
    // e[e] = x[e] - r without a wrap (cofhe_hip_div_close_records: the division and the plaintext addend, on the device from
    // end to end; include/cofhe_hip.h states the contract).  Re-randomised in PerElement mode.
    Tensor<CipherText *> div_close_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &e, const Tensor<PlainText *> &div,
                                                     const Tensor<CipherText *> &rq) const {
        if (rq.num_elements() != e.num_elements()) throw std::invalid_argument("Tensor shapes must be equal");
        DeviceTensor out = div_close_ciphertext_tensor(e, div, upload(rq));
        rerandomize_result(pk, out);
        return download(std::move(out));
    }
    // the same on a resident [r_q]; deterministic
    DeviceTensor div_close_ciphertext_tensor(const Tensor<PlainText *> &e, const Tensor<PlainText *> &div, const DeviceTensor &rq) const {
        const size_t E = e.num_elements(), nd = div.num_elements();
        if (rq.n_ != E) throw std::invalid_argument("Tensor shapes must be equal");
        check_divisors(div, E);
        Staged de = stage(pack_exponents(e)), dd = stage(pack_exponents(div));
        DeviceTensor out = alloc(shape_of(e), E);
        check(cofhe_hip_div_close_records(ctx_, de.ptr, dd.ptr, nd, rq.ptr_, f_rec_.data(), out.ptr_, E, k_, nullptr));
        return out;
    }
    // ---- exact floor division by small public divisors from one opened value (cofhe_hip_divx_*; include/cofhe_hip.h states the
    // protocol and the caller's contract) ----
    // check_divisors, and every divisor at most COFHE_HIP_DIVX_MAX_ROWS: one entry of the tuple per remainder.  Returns `rows`,
    // the largest divisor, which is the length of every element's tuple.
    uint32_t check_small_divisors(const Tensor<PlainText *> &div, size_t n) const {
        check_divisors(div, n);
        uint32_t rows = 1;
        for (size_t i = 0; i < div.num_elements(); i++) {
            if (div[i]->nbits() > 13 || mpz_get_ui(div[i]->get()) > COFHE_HIP_DIVX_MAX_ROWS)
                throw std::invalid_argument("divisors of an exact division: 1 <= D <= 4096; chain factors for more");
            rows = std::max<uint32_t>(rows, (uint32_t)mpz_get_ui(div[i]->get()));
        }
        return rows;
    }
    // {q, m}: q[e] = floor(s(v[e]) / D) mod 2^k and m[e] = s(v[e]) - D q(v[e]) in [0, D) for D = div[e mod count], both of v's
    // shape (cofhe_hip_divmod_plain_records, k_plain_divmod)
    Vector<Tensor<PlainText *>> divmod_plaintext_tensor(const Tensor<PlainText *> &v, const Tensor<PlainText *> &div) const {
        const size_t E = v.num_elements(), nd = div.num_elements();
        const uint32_t rows = check_small_divisors(div, E);
        Staged dv = stage(pack_exponents(v)), dd = stage(pack_exponents(div)), dq = device_buffer(E * EXPW * 4), dm = device_buffer(E * 4);
        check(cofhe_hip_divmod_plain_records(ctx_, dv.ptr, dd.ptr, nd, dq.ptr, dm.ptr, E, rows, k_, nullptr));
        Vector<Tensor<PlainText *>> out;
        out.push_back(read_plaintexts(dq.ptr, E, EXPW, shape_of(v), false));
        std::vector<uint32_t> m(E);
        check(cofhe_hip_download(ctx_, m.data(), dm.ptr, E * 4, nullptr));
        Tensor<PlainText *> rem(shape_of(v), nullptr);
        for (size_t i = 0; i < E; i++) rem[i] = new PlainText((unsigned long)m[i]);
        out.push_back(rem);
        return out;
    }
    // the plaintext rows of the exact-division tuples: res[i, j] = q(r[i]) + [m(r[i]) + j >= D_i] mod 2^k for j < D_i and 0 up to
    // rows, a tensor [n, rows] for the n masks r (cofhe_hip_divx_rows_records: k_divx_prep, k_divx_rows)
    Tensor<PlainText *> divx_rows_plaintext_tensor(const Tensor<PlainText *> &r, const Tensor<PlainText *> &div) const {
        const size_t n = r.num_elements(), nd = div.num_elements();
        const uint32_t rows = check_small_divisors(div, n);
        Staged dr = stage(pack_exponents(r)), dd = stage(pack_exponents(div)), drows = device_buffer(n * rows * EXPW * 4);
        check(cofhe_hip_divx_rows_records(ctx_, dr.ptr, dd.ptr, nd, drows.ptr, n, rows, k_, nullptr));
        return read_plaintexts(drows.ptr, n * rows, EXPW, {n, (size_t)rows}, false);
    }
    // the entries of the exact-division tuples: res[i, j] = a FRESH encryption of row j of element i, a tensor [n, rows]
    // (cofhe_hip_divx_tuples_records: the rows and the fresh-randomness comb, on the device from end to end).  Every entry has
    // its own randomness WHATEVER the randomness mode: the rows differ by 0 or 1, so a shared r would give m(r) away.
    Tensor<CipherText *> divx_tuples_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &div, const Tensor<PlainText *> &r) const {
        const size_t n = r.num_elements(), nd = div.num_elements();
        const uint32_t rows = check_small_divisors(div, n);
        Staged dr = stage(pack_exponents(r)), dd = stage(pack_exponents(div)), drho = stage(draw_randomness(n * rows));
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        DeviceTensor out = alloc(std::vector<size_t>{n, (size_t)rows}, n * rows);
        check(cofhe_hip_divx_tuples_records(ctx_, dr.ptr, dd.ptr, nd, drho.ptr, h_rec_.data(), pkrec.data(), f_rec_.data(), out.ptr_, n, rows, k_,
                                            nullptr));
        return download(std::move(out));
    }
    // the closing step of an exact division: res[i] = (c1, c2 o f^(q(e[i]))) of tuples[i, m(e[i])], of e's shape -- an encryption
    // of floor(s(x[i]) / D) when the tuple is the element's and e[i] = x[i] - r without a wrap (cofhe_hip_divx_close_records: the
    // division, the copy and the plaintext addend, on the device from end to end).  Re-randomised in PerElement mode.
    Tensor<CipherText *> divx_close_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &e, const Tensor<PlainText *> &div,
                                                      const Tensor<CipherText *> &tuples) const {
        DeviceTensor out = divx_close_ciphertext_tensor(e, div, upload(tuples));
        rerandomize_result(pk, out);
        return download(std::move(out));
    }
    // the same on resident tuples; deterministic
    DeviceTensor divx_close_ciphertext_tensor(const Tensor<PlainText *> &e, const Tensor<PlainText *> &div, const DeviceTensor &tuples) const {
        const size_t E = e.num_elements(), nd = div.num_elements();
        const uint32_t rows = check_small_divisors(div, E);
        if (E == 0 || tuples.n_ != E * rows) throw std::invalid_argument("exact-division tuples: one entry per remainder of the largest divisor");
        Staged de = stage(pack_exponents(e)), dd = stage(pack_exponents(div));
        DeviceTensor out = alloc(shape_of(e), E);
        check(cofhe_hip_divx_close_records(ctx_, de.ptr, dd.ptr, nd, tuples.ptr_, rows, f_rec_.data(), out.ptr_, E, k_, nullptr));
        return out;
    }
    // ---- table lookups from one opened value (cofhe_hip_lut_*; include/cofhe_hip.h states the protocol) ----
    // the width b of a public lookup table for n elements: `table` is [2^b] (one table) or [n_tab, 2^b] (element i takes table
    // i mod n_tab, n a multiple of n_tab), 1 <= b <= COFHE_HIP_LUT_MAX_BITS, b <= k
    uint32_t lut_table_bits(const Tensor<PlainText *> &table, size_t n) const {
        if (table.is_zero_degree() || table.ndim() < 1 || table.ndim() > 2) throw std::invalid_argument("lookup table: [2^b] or [n_tab, 2^b]");
        return lut_bits(table.shape().back(), table.num_elements() / (table.shape().back() ? table.shape().back() : 1), n);
    }
    // the plaintext rows of the lookup tuples: res[i, j] = table[i mod n_tab, (j + r[i]) mod 2^b], a tensor [n, 2^b] for the n
    // masks r (cofhe_hip_lut_rotate_records, k_lut_rotate); entries are copied as they are, sign included
    Tensor<PlainText *> lut_rotate_plaintext_tensor(const Tensor<PlainText *> &table, const Tensor<PlainText *> &r) const {
        const size_t n = r.num_elements();
        const uint32_t b = lut_table_bits(table, n);
        const size_t n_tab = table.num_elements() >> b;
        Staged dt = stage(pack_exponents(table)), dr = stage(pack_exponents(r)), drows = device_buffer((n << b) * EXPW * 4);
        check(cofhe_hip_lut_rotate_records(ctx_, dt.ptr, n_tab, dr.ptr, drows.ptr, n, b, nullptr));
        return read_plaintexts(drows.ptr, n << b, EXPW, {n, (size_t)1 << b}, true);
    }
    // the entries of the lookup tuples: res[i, j] = a FRESH encryption of table[i mod n_tab, (j + r[i]) mod 2^b], a tensor
    // [n, 2^b] (cofhe_hip_lut_tuples_records: the rotation and the fresh-randomness comb, on the device from end to end).  Every
    // entry has its own randomness WHATEVER the randomness mode: under a shared r the tuple would give the rotation away.
    Tensor<CipherText *> lut_tuples_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &table, const Tensor<PlainText *> &r) const {
        const size_t n = r.num_elements();
        const uint32_t b = lut_table_bits(table, n);
        const size_t n_tab = table.num_elements() >> b;
        Staged dt = stage(pack_exponents(table)), dr = stage(pack_exponents(r)), drho = stage(draw_randomness(n << b));
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        DeviceTensor out = alloc(std::vector<size_t>{n, (size_t)1 << b}, n << b);
        check(cofhe_hip_lut_tuples_records(ctx_, dt.ptr, n_tab, dr.ptr, drho.ptr, h_rec_.data(), pkrec.data(), f_rec_.data(), out.ptr_, n, b, k_, nullptr));
        return download(std::move(out));
    }
    // encrypt_tensor with its own randomness per ciphertext WHATEVER the randomness mode: the masks [r] of the lookup tuples
    Tensor<CipherText *> encrypt_tensor_per_element(const PublicKey &pk, const Tensor<PlainText *> &pts) const { return encrypt_tensor_fresh(pk, pts); }
    // the closing step of a lookup: res[i] = tuples[i, e[i] mod 2^b], of e's shape, for the opened values e = x - r and the
    // tuple entries [n, 2^b] of the masks r (cofhe_hip_lut_select_records: a copy).  The result is a fresh ciphertext already,
    // so it gets no re-randomisation pass in any mode.
    Tensor<CipherText *> lut_select_ciphertext_tensor(const Tensor<PlainText *> &e, const Tensor<CipherText *> &tuples) const {
        return download(lut_select_ciphertext_tensor(e, upload(tuples)));
    }
    // the same on resident tuples
    DeviceTensor lut_select_ciphertext_tensor(const Tensor<PlainText *> &e, const DeviceTensor &tuples) const {
        const size_t E = e.num_elements();
        if (E == 0 || tuples.n_ % E != 0) throw std::invalid_argument("lookup tuples: 2^b entries for every opened value");
        const uint32_t b = lut_bits(tuples.n_ / E, 1, E);
        Staged de = stage(pack_exponents(e));
        DeviceTensor out = alloc(shape_of(e), E);
        check(cofhe_hip_lut_select_records(ctx_, de.ptr, tuples.ptr_, out.ptr_, E, b, nullptr));
        return out;
    }

    // ---- piecewise-polynomial activations from one opened value (cofhe_hip_spline_*; include/cofhe_hip.h states the protocol
    // and the caller's contract; spline_table.hpp builds tables) ----
    // the degree d and the table count of a spline table for n elements: `table` is [2^bits, d + 1] (one table) or [n_tab, 2^bits,
    // d + 1] (element i takes table i mod n_tab, n a multiple of n_tab); bits >= 1, 1 <= d <= 8, 2^bits (d + 1) <= 4096,
    // shift + bits <= k
    struct SplineShape {
        uint32_t d;
        size_t n_tab;
    };
    SplineShape spline_table_shape(const Tensor<PlainText *> &table, size_t n, uint32_t bits, uint32_t shift) const {
        if (table.is_zero_degree() || table.ndim() < 2 || table.ndim() > 3) throw std::invalid_argument("spline table: [2^bits, d + 1] or [n_tab, 2^bits, d + 1]");
        const size_t pieces = table.shape()[table.ndim() - 2], coefs = table.shape().back();
        if (bits == 0 || bits > 12 || pieces != (size_t)1 << bits || coefs < 2 || coefs > COFHE_HIP_POLY_MAX_DEGREE + 1 ||
            (coefs << bits) > COFHE_HIP_SPLINE_MAX_TUPLE || (size_t)shift + bits > k_)
            throw std::invalid_argument("spline table: 2^bits pieces of d + 1 coefficients, bits >= 1, 1 <= d <= 8, 2^bits (d + 1) <= 4096, shift + bits <= k");
        const size_t n_tab = table.ndim() == 3 ? table.shape()[0] : 1;
        if (n_tab == 0 || n % n_tab != 0) throw std::invalid_argument("spline tables: their count must divide the element count");
        return SplineShape{(uint32_t)coefs - 1, n_tab};
    }
    // the plaintext rows of the spline tuples: res[i, j, .] = the Taylor shift of piece (j + rho_i) mod 2^bits at r[i] minus the
    // piece's origin, a tensor [n, 2^bits, d + 1] for the n masks r (cofhe_hip_spline_rows_records, k_spline_rows)
    Tensor<PlainText *> spline_rows_plaintext_tensor(const Tensor<PlainText *> &table, const Tensor<PlainText *> &r, uint32_t bits, uint32_t shift) const {
        const size_t n = r.num_elements();
        const SplineShape s = spline_table_shape(table, n, bits, shift);
        const size_t per = (size_t)(s.d + 1) << bits;
        Staged dt = stage(pack_exponents(table)), dr = stage(pack_exponents(r)), drows = device_buffer(n * per * EXPW * 4);
        check(cofhe_hip_spline_rows_records(ctx_, dt.ptr, s.n_tab, dr.ptr, drows.ptr, n, bits, shift, s.d, k_, nullptr));
        return read_plaintexts(drows.ptr, n * per, EXPW, {n, (size_t)1 << bits, (size_t)s.d + 1}, true);
    }
    // the entries of the spline tuples: FRESH encryptions of those rows, a tensor [n, 2^bits, d + 1]
    // (cofhe_hip_spline_tuples_records: the rows and the fresh-randomness comb, on the device from end to end).  Every entry has
    // its own randomness WHATEVER the randomness mode: under a shared r the tuple would give the rotation away.
    Tensor<CipherText *> spline_tuples_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &table, const Tensor<PlainText *> &r,
                                                         uint32_t bits, uint32_t shift) const {
        const size_t n = r.num_elements();
        const SplineShape s = spline_table_shape(table, n, bits, shift);
        const size_t per = (size_t)(s.d + 1) << bits;
        Staged dt = stage(pack_exponents(table)), dr = stage(pack_exponents(r)), drho = stage(draw_randomness(n * per));
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        DeviceTensor out = alloc(std::vector<size_t>{n, (size_t)1 << bits, (size_t)s.d + 1}, n * per);
        check(cofhe_hip_spline_tuples_records(ctx_, dt.ptr, s.n_tab, dr.ptr, drho.ptr, h_rec_.data(), pkrec.data(), f_rec_.data(), out.ptr_, n, bits,
                                              shift, s.d, k_, nullptr));
        return download(std::move(out));
    }
    // the closing step of a spline: res[i] = [q_{j,0}] o prod_c [q_{j,c}]^(e[i]^c), j the segment of e[i], of e's shape, for the
    // opened values e = x - r and the tuple entries [n, 2^bits, d + 1] of the masks r (cofhe_hip_spline_close_records).  Its
    // randomness is the tuple entries' own, so it gets no re-randomisation pass in any mode.
    Tensor<CipherText *> spline_close_ciphertext_tensor(const Tensor<PlainText *> &e, const Tensor<CipherText *> &tuples, uint32_t bits,
                                                        uint32_t shift) const {
        return download(spline_close_ciphertext_tensor(e, upload(tuples), bits, shift));
    }
    // the same on resident tuples
    DeviceTensor spline_close_ciphertext_tensor(const Tensor<PlainText *> &e, const DeviceTensor &tuples, uint32_t bits, uint32_t shift) const {
        const size_t E = e.num_elements();
        if (E == 0 || bits == 0 || bits > 12 || tuples.n_ % (E << bits) != 0 || tuples.n_ / (E << bits) < 2)
            throw std::invalid_argument("spline tuples: 2^bits rows of d + 1 entries for every opened value");
        const uint32_t d = (uint32_t)(tuples.n_ / (E << bits)) - 1;
        Staged de = stage(pack_exponents(e));
        DeviceTensor out = alloc(shape_of(e), E);
        check(cofhe_hip_spline_close_records(ctx_, de.ptr, tuples.ptr_, out.ptr_, E, bits, shift, d, k_, nullptr));
        return out;
    }

    // ---- the sign on a window of up to 64 bits from digit comparisons (cofhe_hip_cmp_*; include/cofhe_hip.h states the protocol) ----
    // n = ceil(bits / digit_bits) digits and n 2^digit_bits entries per element; refuses what cofhe_hip_cmp_shape refuses
    struct CmpShape {
        uint32_t digits, entries;
    };
    CmpShape cmp_shape(uint32_t bits, uint32_t digit_bits) const {
        CmpShape s{0, 0};
        check(cofhe_hip_cmp_shape(bits, digit_bits, k_, 0, nullptr, 0, nullptr, &s.digits, &s.entries));
        return s;
    }
    // the digit width for a window of `bits` bits that needs the fewest ciphertexts per element: n 2^d of the comparison tuple
    // and 2 2^(n + 1) of the two lookups that close it; the smallest such d, 0 when the bounds allow none
    uint32_t cmp_pick_digit_bits(uint32_t bits) const {
        uint32_t best = 0;
        uint64_t best_cost = 0;
        for (uint32_t d = 1; d <= COFHE_HIP_CMP_MAX_DIGIT_BITS; d++) {
            uint32_t n = 0;
            if (cofhe_hip_cmp_shape(bits, d, k_, 0, nullptr, 0, nullptr, &n, nullptr) != COFHE_HIP_OK) continue;
            const uint64_t cost = ((uint64_t)n << d) + ((uint64_t)1 << (n + 2));
            if (best == 0 || cost < best_cost) {
                best = d;
                best_cost = cost;
            }
        }
        return best;
    }
    // the plaintext rows of the comparison tuples: res[i, j, c] = 2^j sgn(r_ij - c), r_ij digit j of r[i] mod 2^bits, a tensor
    // [n, digits, 2^digit_bits] for the n masks r (cofhe_hip_cmp_rows_records, k_cmp_rows)
    Tensor<PlainText *> cmp_rows_plaintext_tensor(const Tensor<PlainText *> &r, uint32_t bits, uint32_t digit_bits) const {
        const size_t n = r.num_elements();
        const CmpShape s = cmp_shape(bits, digit_bits);
        Staged dr = stage(pack_exponents(r)), drows = device_buffer(n * s.entries * EXPW * 4);
        check(cofhe_hip_cmp_rows_records(ctx_, dr.ptr, drows.ptr, n, bits, digit_bits, k_, nullptr));
        return read_plaintexts(drows.ptr, n * s.entries, EXPW, {n, (size_t)s.digits, (size_t)1 << digit_bits}, true);
    }
    // the entries of the comparison tuples: FRESH encryptions of those rows, a tensor [n, digits, 2^digit_bits]
    // (cofhe_hip_cmp_tuples_records: the rows and the fresh-randomness comb, on the device from end to end).  Every entry has
    // its own randomness WHATEVER the randomness mode: under a shared r the tuple would give the digits of the mask away.
    Tensor<CipherText *> cmp_tuples_ciphertext_tensor(const PublicKey &pk, const Tensor<PlainText *> &r, uint32_t bits, uint32_t digit_bits) const {
        const size_t n = r.num_elements();
        const CmpShape s = cmp_shape(bits, digit_bits);
        Staged dr = stage(pack_exponents(r)), drho = stage(draw_randomness(n * s.entries));
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        DeviceTensor out = alloc(std::vector<size_t>{n, (size_t)s.digits, (size_t)1 << digit_bits}, n * s.entries);
        check(cofhe_hip_cmp_tuples_records(ctx_, dr.ptr, drho.ptr, h_rec_.data(), pkrec.data(), f_rec_.data(), out.ptr_, n, bits, digit_bits, k_, nullptr));
        return download(std::move(out));
    }
    // the closing step of a comparison's first round, for the opened values e = x - r and the tuple entries [n, digits,
    // 2^digit_bits] of the masks r: pairs[i, 0] = [S_A], pairs[i, 1] = [S_B], the products of the entries that the two thresholds
    // of e[i] mod 2^bits select, and wrap[i] = [A > B] (cofhe_hip_cmp_close_records).  The pairs carry the randomness of the
    // entries they are products of, so they get no re-randomisation pass in any mode.
    struct CmpClosed {
        Tensor<CipherText *> pairs;          // [n, 2]
        Tensor<PlainText *> wrap;            // [n]
    };
    CmpClosed cmp_close_ciphertext_tensor(const Tensor<PlainText *> &e, const Tensor<CipherText *> &tuples, uint32_t bits, uint32_t digit_bits) const {
        return cmp_close_ciphertext_tensor(e, upload(tuples), bits, digit_bits);
    }
    // the same on resident tuples
    CmpClosed cmp_close_ciphertext_tensor(const Tensor<PlainText *> &e, const DeviceTensor &tuples, uint32_t bits, uint32_t digit_bits) const {
        const size_t E = e.num_elements();
        const CmpShape s = cmp_shape(bits, digit_bits);
        if (E == 0 || tuples.n_ != E * s.entries) throw std::invalid_argument("comparison tuples: ceil(bits / d) 2^d entries for every opened value");
        Staged de = stage(pack_exponents(e)), dwrap = device_buffer(E * EXPW * 4);
        DeviceTensor out = alloc(std::vector<size_t>{E, 2}, 2 * E);
        check(cofhe_hip_cmp_close_records(ctx_, de.ptr, tuples.ptr_, out.ptr_, dwrap.ptr, E, bits, digit_bits, k_, nullptr));
        Tensor<PlainText *> wrap = read_plaintexts(dwrap.ptr, E, EXPW, {E}, true);
        return CmpClosed{download(std::move(out)), wrap};
    }

    // ---- device-resident variants -------------------------------------------------------------
    // the block behind a tensor whose elements are, in order, ALL the elements of one device block (the result of
    // a previous operation handed back unchanged); nullptr otherwise
    static std::shared_ptr<DeviceBlock> whole_block(const Tensor<CipherText *> &t) {
        const size_t E = t.num_elements();
        if (E == 0 || !t[0]) return nullptr;
        const std::shared_ptr<DeviceBlock> &b = t[0]->block();
        if (!b || b->n_ct != E) return nullptr;
        for (size_t i = 0; i < E; i++)
            if (!t[i] || t[i]->block() != b || t[i]->block_index() != i) return nullptr;
        return b;
    }
    DeviceTensor upload(const Tensor<CipherText *> &t) const {
        const size_t E = t.num_elements();
        if (std::shared_ptr<DeviceBlock> b = whole_block(t)) {
            if (b->ctx == ctx_) {                      // already resident: a view, nothing moves
                DeviceTensor d;
                d.ctx_ = ctx_;
                d.ptr_ = b->dptr;
                d.shape_ = t.shape();                  // empty for a 0-D tensor
                d.n_ = E;
                d.keep_ = b;
                return d;
            }
        }
        if (resident_gather_ && E != 0) {
            DeviceTensor d;
            if (gather_resident(t, d)) return d;
        }
        std::vector<uint32_t> recs(E * 2 * REC, 0);
        pack_forms(2 * E, recs.data(), [&](size_t i) -> const QFI & { const CipherText &e = *t[i >> 1]; return (i & 1) ? e.c2() : e.c1(); });
        DeviceTensor d = alloc(t.shape(), E);
        fill(d, recs);
        return d;
    }
    // The device route of upload(): a tensor that is no whole block, but whose elements are all non-null, not host-dirty and
    // resident in this context, in at most 8 distinct blocks -- a column of a triplet block, a transposed or replicated result,
    // the taps of a pooling window.  One index array per source block (COFHE_HIP_GATHER_KEEP at the elements of the others),
    // staged, and one cofhe_hip_gather_records per block into the one result: no record crosses PCIe and no GMP object is
    // made.  The bytes are those of the host path (set_resident_gather(false)).  The status word is sticky, so a failed
    // computation in a source block is still reported when data next leaves the device.  False: not such a tensor.
    void set_resident_gather(bool on) { resident_gather_ = on; }
    bool resident_gather() const { return resident_gather_; }
    // DeviceBlock record downloads (the whole-block transfer behind the first read of a lazy element, the host path of upload
    // and of serialize) of this cryptosystem's blocks since construction
    uint64_t block_downloads() const { return downloads_->load(std::memory_order_relaxed); }
    bool gather_resident(const Tensor<CipherText *> &t, DeviceTensor &out) const {
        constexpr size_t MAX_BLOCKS = 8;
        const size_t E = t.num_elements();
        std::shared_ptr<DeviceBlock> blocks[MAX_BLOCKS];
        size_t nb = 0;
        std::vector<uint32_t> which(E);
        for (size_t i = 0; i < E; i++) {
            if (!t[i]) return false;
            const std::shared_ptr<DeviceBlock> &b = t[i]->block();
            if (!b || b->ctx != ctx_ || t[i]->block_index() >= b->n_ct || b->n_ct > COFHE_HIP_GATHER_KEEP) return false;
            size_t j = 0;
            while (j < nb && blocks[j] != b) j++;
            if (j == nb) {
                if (nb == MAX_BLOCKS) return false;
                blocks[nb++] = b;
            }
            which[i] = (uint32_t)j;
        }
        out = alloc(t.shape(), E);
        for (size_t j = 0; j < nb; j++) {
            std::vector<uint32_t> index(E, COFHE_HIP_GATHER_KEEP);
            for (size_t i = 0; i < E; i++)
                if (which[i] == j) index[i] = (uint32_t)t[i]->block_index();
            Staged di = stage(std::move(index));
            check(cofhe_hip_gather_records(ctx_, blocks[j]->dptr, blocks[j]->n_ct, di.ptr, nullptr, out.ptr_, E, 2 * REC, nullptr));
        }
        return true;
    }
    // hands the device tensor over to a Tensor<CipherText *> whose elements reference it (no transfer, no GMP work:
    // values appear when somebody reads them); the caller owns the elements as with every other result tensor
    Tensor<CipherText *> download(DeviceTensor &&d) const {
        Tensor<CipherText *> out(d.shape_.empty() ? std::vector<size_t>{d.n_} : d.shape_, nullptr);
        Tensor<CipherText *> flat = out;
        flat.flatten();
        std::shared_ptr<DeviceBlock> blk = d.keep_;
        if (!blk) {
            blk = std::make_shared<DeviceBlock>(ctx_owner_, d.ptr_, d.n_);
            blk->downloads = downloads_;
            d.ptr_ = nullptr;                          // ownership moved into the block
        }
        for (size_t i = 0; i < d.n_; i++) flat[i] = new CipherText(blk, i);
        d.n_ = 0;
        return out;
    }
    // same for a tensor the caller keeps: the records are copied out now (eager GMP objects)
    Tensor<CipherText *> download(const DeviceTensor &d) const {
        std::vector<uint32_t> recs(d.n_ * 2 * REC);
        check(cofhe_hip_download(ctx_, recs.data(), d.ptr_, recs.size() * 4, nullptr));
        DeviceBlock::throw_on_device_status(ctx_);
        Tensor<CipherText *> out(d.shape_.empty() ? std::vector<size_t>{d.n_} : d.shape_, nullptr);
        Tensor<CipherText *> flat = out;
        flat.flatten();
        COFHE_HOST_PARALLEL_FOR
        for (size_t i = 0; i < d.n_; i++)
            flat[i] = new CipherText(unpack_form(&recs[(2 * i) * REC]), unpack_form(&recs[(2 * i + 1) * REC]));
        return out;
    }
    DeviceTensor add_ciphertext_tensors(const DeviceTensor &a, const DeviceTensor &b) const {
        if (a.shape_ != b.shape_) throw std::invalid_argument("Tensor shapes must be equal");
        DeviceTensor r = alloc(a.shape_, a.n_);
        check(cofhe_hip_add_ciphertext_records(ctx_, a.ptr_, b.ptr_, r.ptr_, a.n_, nullptr));
        return r;
    }
    DeviceTensor sub_ciphertext_tensors(const DeviceTensor &a, const DeviceTensor &b) const {
        if (a.shape_ != b.shape_) throw std::invalid_argument("Tensor shapes must be equal");
        DeviceTensor r = alloc(a.shape_, a.n_);
        check(cofhe_hip_sub_ciphertext_records(ctx_, a.ptr_, b.ptr_, r.ptr_, a.n_, nullptr));
        return r;
    }
    // ---- rearranging resident tensors (cofhe_hip_view_records, cofhe_hip_gather_records; include/cofhe_hip.h states the
    // descriptor) ----
    // Every result element is a byte-for-byte COPY of an element of x or of `fill`: nothing is composed and NOTHING IS
    // RE-RANDOMISED, in any randomness mode -- a copy shares its randomness with its source, and c2 o c2'^-1 of the two is the
    // principal form.  A caller that hands both a copy and its original (or two copies) to another party calls
    // rerandomize_ciphertext_tensor on what leaves first.  Each operation exists on DeviceTensor and on Tensor<CipherText *>
    // (upload, operate, hand over: the lazy download that moves nothing).  Shape errors throw std::invalid_argument.
    //
    // the general entry: the view's source is x (the shapes must agree), the result is the view's whole destination, which the
    // view's box must cover (a box inside a larger destination is what concat_ciphertext_tensors issues); `fill`: one element,
    // needed when the view reads outside x
    DeviceTensor view_ciphertext_tensor(const DeviceTensor &x, const cofhe_hip_view &view, const DeviceTensor *fill = nullptr) const {
        uint64_t n_src = 0, n_box = 0, n_dst = 0;
        int needs_fill = 0;
        check(cofhe_hip_view_check(&view, &n_src, &n_box, &n_dst, &needs_fill));
        if (n_box != n_dst) throw std::invalid_argument("view: the box must cover the whole destination");
        DeviceTensor out = alloc(extents(view.dst_extent, view.out_ndim), n_dst);
        view_into(x, view, fill, out);
        return out;
    }
    Tensor<CipherText *> view_ciphertext_tensor(const Tensor<CipherText *> &x, const cofhe_hip_view &view, const CipherText *fill = nullptr) const {
        if (!fill) return download(view_ciphertext_tensor(upload(x), view));
        const DeviceTensor f = upload(Tensor<CipherText *>(1, const_cast<CipherText *>(fill)));
        return download(view_ciphertext_tensor(upload(x), view, &f));
    }
    // result axis d is axis perm[d] of x (numpy.transpose)
    DeviceTensor permute_ciphertext_tensor(const DeviceTensor &x, const std::vector<size_t> &perm) const {
        if (perm.size() != x.shape_.size()) throw std::invalid_argument("permute: one entry per axis");
        std::vector<uint32_t> p(perm.begin(), perm.end());
        for (size_t d = 0; d < perm.size(); d++)
            if (perm[d] >= perm.size()) throw std::invalid_argument("permute: not a permutation of the axes");
        cofhe_hip_view v;
        check(cofhe_hip_view_permute(shape64(x).data(), (uint32_t)perm.size(), p.data(), &v));
        return view_ciphertext_tensor(x, v);
    }
    Tensor<CipherText *> permute_ciphertext_tensor(const Tensor<CipherText *> &x, const std::vector<size_t> &perm) const {
        return download(permute_ciphertext_tensor(upload(x), perm));
    }
    DeviceTensor transpose_ciphertext_tensor(const DeviceTensor &x) const {
        if (x.shape_.size() != 2) throw std::invalid_argument("transpose: a 2-D tensor");
        return permute_ciphertext_tensor(x, {1, 0});
    }
    Tensor<CipherText *> transpose_ciphertext_tensor(const Tensor<CipherText *> &x) const { return download(transpose_ciphertext_tensor(upload(x))); }
    // x[start[0]:stop[0]:step[0], ...]: bounds within their axes, steps != 0; with a negative step a stop of -1 means "down to and
    // including element 0"
    DeviceTensor slice_ciphertext_tensor(const DeviceTensor &x, const std::vector<int64_t> &start, const std::vector<int64_t> &stop,
                                         const std::vector<int64_t> &step) const {
        const size_t nd = x.shape_.size();
        if (start.size() != nd || stop.size() != nd || step.size() != nd) throw std::invalid_argument("slice: one bound and one step per axis");
        cofhe_hip_view v;
        check(cofhe_hip_view_slice(shape64(x).data(), (uint32_t)nd, start.data(), stop.data(), step.data(), &v));
        return view_ciphertext_tensor(x, v);
    }
    Tensor<CipherText *> slice_ciphertext_tensor(const Tensor<CipherText *> &x, const std::vector<int64_t> &start, const std::vector<int64_t> &stop,
                                                 const std::vector<int64_t> &step) const {
        return download(slice_ciphertext_tensor(upload(x), start, stop, step));
    }
    DeviceTensor flip_ciphertext_tensor(const DeviceTensor &x, size_t axis) const {
        const size_t nd = x.shape_.size();
        if (axis >= nd) throw std::invalid_argument("flip: no such axis");
        std::vector<int64_t> start(nd, 0), stop(x.shape_.begin(), x.shape_.end()), step(nd, 1);
        start[axis] = (int64_t)x.shape_[axis] - 1;
        stop[axis] = -1;
        step[axis] = -1;
        return slice_ciphertext_tensor(x, start, stop, step);
    }
    Tensor<CipherText *> flip_ciphertext_tensor(const Tensor<CipherText *> &x, size_t axis) const { return download(flip_ciphertext_tensor(upload(x), axis)); }
    // numpy's rule, right-aligned: every extent of x equals the extent of `shape` it is aligned with, or is 1
    DeviceTensor broadcast_ciphertext_tensor(const DeviceTensor &x, const std::vector<size_t> &shape) const {
        std::vector<uint64_t> out(shape.begin(), shape.end());
        cofhe_hip_view v;
        check(cofhe_hip_view_broadcast(shape64(x).data(), (uint32_t)x.shape_.size(), out.data(), (uint32_t)out.size(), &v));
        return view_ciphertext_tensor(x, v);
    }
    Tensor<CipherText *> broadcast_ciphertext_tensor(const Tensor<CipherText *> &x, const std::vector<size_t> &shape) const {
        return download(broadcast_ciphertext_tensor(upload(x), shape));
    }
    // lo[d] elements of `fill` before and hi[d] after x on every axis
    DeviceTensor pad_ciphertext_tensor(const DeviceTensor &x, const std::vector<size_t> &lo, const std::vector<size_t> &hi, const DeviceTensor &fill) const {
        const size_t nd = x.shape_.size();
        if (lo.size() != nd || hi.size() != nd) throw std::invalid_argument("pad: one width per axis and side");
        std::vector<uint64_t> l(lo.begin(), lo.end()), h(hi.begin(), hi.end());
        cofhe_hip_view v;
        check(cofhe_hip_view_pad(shape64(x).data(), (uint32_t)nd, l.data(), h.data(), &v));
        return view_ciphertext_tensor(x, v, &fill);
    }
    Tensor<CipherText *> pad_ciphertext_tensor(const Tensor<CipherText *> &x, const std::vector<size_t> &lo, const std::vector<size_t> &hi,
                                               const CipherText &fill) const {
        return download(pad_ciphertext_tensor(upload(x), lo, hi, upload(Tensor<CipherText *>(1, const_cast<CipherText *>(&fill)))));
    }
    // the parts side by side along `axis` (their other extents agree): the result is allocated once, and every part is one view
    // call that writes its box
    DeviceTensor concat_ciphertext_tensors(const std::vector<const DeviceTensor *> &parts, size_t axis) const {
        if (parts.empty() || !parts[0]) throw std::invalid_argument("concat: no parts");
        std::vector<size_t> shape = parts[0]->shape_;
        if (axis >= shape.size()) throw std::invalid_argument("concat: no such axis");
        shape[axis] = 0;
        for (const DeviceTensor *p : parts) {
            if (!p || p->shape_.size() != shape.size()) throw std::invalid_argument("Tensor shapes must be equal");
            for (size_t d = 0; d < shape.size(); d++)
                if (d != axis && p->shape_[d] != shape[d]) throw std::invalid_argument("Tensor shapes must be equal");
            shape[axis] += p->shape_[axis];
        }
        size_t n = 1;
        for (size_t e : shape) n *= e;
        DeviceTensor out = alloc(shape, n);
        std::vector<uint64_t> dst(shape.begin(), shape.end()), at(shape.size(), 0);
        std::vector<uint32_t> ident(shape.size());
        for (size_t d = 0; d < ident.size(); d++) ident[d] = (uint32_t)d;
        for (const DeviceTensor *p : parts) {
            cofhe_hip_view v;
            check(cofhe_hip_view_permute(shape64(*p).data(), (uint32_t)ident.size(), ident.data(), &v));
            check(cofhe_hip_view_into(&v, dst.data(), at.data()));
            view_into(*p, v, nullptr, out);
            at[axis] += p->shape_[axis];
        }
        return out;
    }
    Tensor<CipherText *> concat_ciphertext_tensors(const Vector<Tensor<CipherText *>> &parts, size_t axis) const {
        std::vector<DeviceTensor> held;
        held.reserve(parts.size());
        for (const Tensor<CipherText *> &p : parts) held.push_back(upload(p));
        std::vector<const DeviceTensor *> ptrs;
        for (const DeviceTensor &d : held) ptrs.push_back(&d);
        return download(concat_ciphertext_tensors(ptrs, axis));
    }
    // the taps of every pooling / convolution window of x [B, H, W, C]: [kh, kw, B, Ho, Wo, C], `fill` in the padding (needed when a
    // pad is not 0)
    DeviceTensor window_taps_ciphertext_tensor(const DeviceTensor &x, const std::array<size_t, 2> &kernel, const std::array<size_t, 2> &stride,
                                               const std::array<size_t, 2> &pad = {0, 0}, const std::array<size_t, 2> &dilation = {1, 1},
                                               const DeviceTensor *fill = nullptr) const {
        if (x.shape_.size() != 4) throw std::invalid_argument("window taps: the image is [B, H, W, C]");
        const cofhe_hip_conv2d_geometry g = conv_geometry({x.shape_[0], x.shape_[1], x.shape_[2], x.shape_[3], kernel[0], kernel[1], x.shape_[3],
                                                           stride[0], stride[1], pad[0], pad[1], dilation[0], dilation[1], 1});
        cofhe_hip_view v;
        check(cofhe_hip_view_window_taps(&g, &v));
        return view_ciphertext_tensor(x, v, fill);
    }
    Tensor<CipherText *> window_taps_ciphertext_tensor(const Tensor<CipherText *> &x, const std::array<size_t, 2> &kernel,
                                                       const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad = {0, 0},
                                                       const std::array<size_t, 2> &dilation = {1, 1}, const CipherText *fill = nullptr) const {
        if (!fill) return download(window_taps_ciphertext_tensor(upload(x), kernel, stride, pad, dilation));
        const DeviceTensor f = upload(Tensor<CipherText *>(1, const_cast<CipherText *>(fill)));
        return download(window_taps_ciphertext_tensor(upload(x), kernel, stride, pad, dilation, &f));
    }
    // res[i] = x[indices[i]] over the elements of x in row-major order, a 1-D tensor; an index of COFHE_HIP_GATHER_FILL takes
    // `fill`.  An index beyond x is refused here, before anything runs.
    DeviceTensor gather_ciphertext_tensor(const DeviceTensor &x, const std::vector<uint32_t> &indices, const DeviceTensor *fill = nullptr) const {
        for (uint32_t ix : indices) {
            if (ix == COFHE_HIP_GATHER_FILL ? fill == nullptr : ix >= x.n_)
                throw std::invalid_argument(ix == COFHE_HIP_GATHER_FILL ? "gather: a fill index and no fill element" : "gather: an index beyond the tensor");
        }
        if (fill && fill->n_ != 1) throw std::invalid_argument("gather: the fill is one element");
        DeviceTensor out = alloc({indices.size()}, indices.size());
        if (indices.empty()) return out;
        Staged di = stage(std::vector<uint32_t>(indices));
        check(cofhe_hip_gather_records(ctx_, x.ptr_, x.n_, di.ptr, fill ? fill->ptr_ : nullptr, out.ptr_, indices.size(), 2 * REC, nullptr));
        return out;
    }
    Tensor<CipherText *> gather_ciphertext_tensor(const Tensor<CipherText *> &x, const std::vector<uint32_t> &indices, const CipherText *fill = nullptr) const {
        if (!fill) return download(gather_ciphertext_tensor(upload(x), indices));
        const DeviceTensor f = upload(Tensor<CipherText *>(1, const_cast<CipherText *>(fill)));
        return download(gather_ciphertext_tensor(upload(x), indices, &f));
    }
    void synchronize() const { check(cofhe_hip_stream_sync(ctx_, nullptr)); }

    // ---- binary tensor format (reference: cpu_cryptosystem.inl:320-508) ------------------------
    String serialize_ciphertext_tensor(const Tensor<CipherText *> &t) const {
        const size_t E = t.num_elements();
        std::vector<uint32_t> shape(t.shape().begin(), t.shape().end());
        std::shared_ptr<DeviceBlock> b = whole_block(t);
        if (b && b->ctx == ctx_) {
            // resident result: the wire format is written by the GPU (wire.hip) and only those bytes cross PCIe
            const size_t cap = cofhe_hip_packed_size_bound(E * 2, 2, (uint32_t)shape.size());
            Staged dby = device_buffer(cap);
            size_t len = 0;
            check(cofhe_hip_pack_tensor_device(ctx_, b->dptr, E * 2, 2, (uint32_t)shape.size(), shape.data(), dby.ptr, cap, &len, nullptr));
            String s(len, '\0');
            check(cofhe_hip_download(ctx_, &s[0], dby.ptr, len, nullptr));
            DeviceBlock::throw_on_device_status(ctx_);       // the bytes leave the process: never with a cap bit set
            return s;
        }
        std::vector<uint32_t> packed;
        const uint32_t *recs = nullptr;
        if (b) {
            recs = b->records();                        // one download, no GMP objects
        } else {
            packed.assign(E * 2 * REC, 0);
            pack_forms(2 * E, packed.data(), [&](size_t i) -> const QFI & { const CipherText &e = *t[i >> 1]; return (i & 1) ? e.c2() : e.c1(); });
            recs = packed.data();
        }
        uint8_t *bytes = nullptr;
        size_t len = 0;
        check(cofhe_hip_records_to_bytes(recs, E * 2, (uint32_t)shape.size(), shape.data(), &bytes, &len));
        String s((const char *)bytes, len);
        cofhe_hip_host_free(bytes);
        return s;
    }
    // The bytes go to the GPU as they are; wire.hip turns them into records there and checks that every form is a
    // reduced form of this discriminant (a forged tensor is refused, cofhe_hip.h).  The elements of the result
    // reference the resident block; GMP values appear when somebody reads them.
    Tensor<CipherText *> deserialize_ciphertext_tensor(const String &data) const {
        if (data.size() < 4) throw std::invalid_argument("tensor buffer too short");
        uint32_t nd = 0;
        memcpy(&nd, data.data(), 4);
        if (nd == 0 || nd > 8 || data.size() < 4 + 4ull * nd) return deserialize_ciphertext_tensor_host(data);
        uint64_t E = 1;
        std::vector<size_t> sh(nd);
        for (uint32_t i = 0; i < nd; i++) {
            uint32_t dim = 0;
            memcpy(&dim, data.data() + 4 + 4 * i, 4);
            sh[i] = dim;
            if (dim != 0 && E > (1ull << 40) / dim) throw std::invalid_argument("tensor too large");
            E *= dim;
        }
        if (E == 0 || data.size() < 4 + 4ull * nd + 16 * E) return deserialize_ciphertext_tensor_host(data);      // the host parser words the error
        Staged dby = device_buffer(data.size());
        check(cofhe_hip_upload(ctx_, dby.ptr, data.data(), data.size(), nullptr));      // the caller's bytes: they outlive dby
        DeviceTensor d = alloc(sh, E);
        uint32_t ndim = 0, shape[8];
        uint64_t n = 0;
        check(cofhe_hip_unpack_tensor_device(ctx_, dby.ptr, data.size(), 2, d.ptr_, E * 2, &ndim, shape, &n, nullptr));
        return download(std::move(d));
    }
    Tensor<CipherText *> deserialize_ciphertext_tensor_host(const String &data) const {
        uint32_t ndim = 0, shape[8];
        uint32_t *recs = nullptr;
        uint64_t n = 0;
        check(cofhe_hip_bytes_to_records((const uint8_t *)data.data(), data.size(), &ndim, shape, &recs, &n));
        std::vector<size_t> sh(shape, shape + ndim);
        Tensor<CipherText *> out(sh, nullptr);
        Tensor<CipherText *> flat = out;
        flat.flatten();
        COFHE_HOST_PARALLEL_FOR
        for (uint64_t i = 0; i < n / 2; i++)
            flat[i] = new CipherText(unpack_form(recs + (2 * i) * REC), unpack_form(recs + (2 * i + 1) * REC));
        cofhe_hip_host_free(recs);
        return out;
    }

    // base^e through the context's fixed-base table of `base` (h, public keys)
    QFI pow_fixed_base(const QFI &base, const Mpz &e) const {
        const std::array<uint32_t, REC> b = record_of(base);
        const std::vector<uint32_t> x = exponent_record(e);
        Staged dout = device_buffer(REC * 4);
        check(cofhe_hip_pow_fixed_base_record(ctx_, b.data(), x.data(), dout.ptr, nullptr));
        return read_forms(dout.ptr, 1)[0];
    }
    // form-level helpers (also used by the tests): element-wise powers / products on the GPU
    std::vector<QFI> pow_forms(const std::vector<QFI> &bases, const std::vector<Mpz> &exps) const {
        const size_t n = bases.size();
        std::vector<uint32_t> recs(n * REC, 0), ex(n * EXPW, 0);
        for (size_t i = 0; i < n; i++) {
            pack_form(bases[i], &recs[i * REC]);
            pack_exponent(exps[i], &ex[i * EXPW]);
        }
        Staged db = stage(std::move(recs)), de = stage(std::move(ex)), dout = device_buffer(n * REC * 4);
        check(cofhe_hip_pow_form_records(ctx_, db.ptr, de.ptr, dout.ptr, n, nullptr));
        return read_forms(dout.ptr, n);
    }
    std::vector<QFI> compose_forms(const std::vector<QFI> &x, const std::vector<QFI> &y) const {
        const size_t n = x.size();
        std::vector<uint32_t> rx(n * REC, 0), ry(n * REC, 0);
        for (size_t i = 0; i < n; i++) {
            pack_form(x[i], &rx[i * REC]);
            pack_form(y[i], &ry[i * REC]);
        }
        Staged dx = stage(std::move(rx)), dy = stage(std::move(ry)), dout = device_buffer(n * REC * 4);
        check(cofhe_hip_compose_records(ctx_, dx.ptr, dy.ptr, dout.ptr, n, nullptr));
        return read_forms(dout.ptr, n);
    }

    // ---- text formats of single values (reference: cpu_cryptosystem.inl:124-227): decimal integers separated by
    // blanks, "a b c" per form, c1 then c2 for a ciphertext
    String serialize_plaintext(const PlainText &s) const { return s.str(); }
    PlainText deserialize_plaintext(const String &data) const { return parse_mpz(first_tokens(data, 1)[0]); }
    String serialize_secret_key(const SecretKey &sk) const { return sk.str(); }
    SecretKey deserialize_secret_key(const String &data) const { return parse_mpz(first_tokens(data, 1)[0]); }
    String serialize_secret_key_share(const SecretKeyShare &sks) const { return sks.str(); }
    SecretKeyShare deserialize_secret_key_share(const String &data) const { return parse_mpz(first_tokens(data, 1)[0]); }
    String serialize_public_key(const PublicKey &pk) const { return form_text(pk); }
    PublicKey deserialize_public_key(const String &data) const { return form_from(first_tokens(data, 3), 0); }
    String serialize_part_decryption_result(const PartDecryptionResult &pdr) const { return form_text(pdr); }
    PartDecryptionResult deserialize_part_decryption_result(const String &data) const { return form_from(first_tokens(data, 3), 0); }
    String serialize_ciphertext(const CipherText &ct) const { return form_text(ct.c1()) + " " + form_text(ct.c2()); }
    CipherText deserialize_ciphertext(const String &data) const {
        const std::vector<std::string> t = first_tokens(data, 6);
        return CipherText(form_from(t, 0), form_from(t, 3));
    }
    // "HIPCryptoSystem <sec> <k> <compact>" (the reference writes its own class name: cpu_cryptosystem.inl:124-127)
    String serialize() const { return "HIPCryptoSystem " + std::to_string(sec_level_) + " " + std::to_string(k_) + " 0"; }
    // what the reference's static deserialize does (cpu_cryptosystem.inl:129-137): reads "<type> <sec> <k> <compact>" and
    // constructs a system of those sizes (the text carries no parameters; the compact variant does not exist here)
    static HIPCryptoSystem deserialize(const String &data) {
        std::istringstream ss{data};
        String type;
        int sec_level = 0, k = 0;
        bool compact_variant = false;
        ss >> type >> sec_level >> k >> compact_variant;
        if (!ss || sec_level <= 0 || k <= 0) throw std::invalid_argument("malformed cryptosystem description");
        if (compact_variant) throw std::invalid_argument("the compact variant is not supported (the reference hard-codes compact = false)");
        return HIPCryptoSystem((uint32_t)sec_level, (uint32_t)k);
    }

    // ---- the class-group handles the node layer reaches through (reference: get_hsm2k().Cl_G() / Cl_Delta(),
    // cpu_cryptosystem.hpp:139, used as cl_g.nucomp(r, f1, f2) at include/smpc/ciphertext_multiplications.hpp:85-98).
    // Non-compact mode: both are the class group of Delta.  nucomp / nudupl / nupow run on the GPU; the batched forms
    // take whole vectors in one launch (one composition per call is a 0.4 ms round trip).
    class ClassGroupHandle {
      public:
        explicit ClassGroupHandle(const HIPCryptoSystem *cs) : cs_(cs) {}
        const Mpz &discriminant() const { return cs_->delta_; }
        Mpz default_nucomp_bound() const {        // floor(|Delta|^(1/4)), what BICYCL's ClassGroup caches (unused by the kernels)
            Mpz ad = cs_->delta_, r;
            ad.neg();
            mpz_root(r.get(), ad.get(), 4);
            return r;
        }
        QFI one() const {
            Mpz a(1ul), b, c, t;
            const unsigned long par = mpz_tstbit(cs_->delta_.get(), 0) ? 1ul : 0ul;     // Delta mod 4 in {0, 1}
            mpz_set_ui(b.get(), par);
            mpz_ui_sub(c.get(), par, cs_->delta_.get());
            mpz_fdiv_q_2exp(c.get(), c.get(), 2);
            return QFI(a, b, c);
        }
        void nucomp(QFI &r, const QFI &f1, const QFI &f2) const { r = cs_->compose_forms({f1}, {f2})[0]; }
        void nucompinv(QFI &r, const QFI &f1, const QFI &f2) const {
            // inverse of a reduced form: (a, -b, c), except on the boundary of the reduced domain (b == a or a == c),
            // where (a, b, c) is its own reduced inverse representative
            Mpz nb = f2.b();
            if (!(f2.b() == f2.a()) && !(f2.a() == f2.c())) nb.neg();
            r = cs_->compose_forms({f1}, {QFI(f2.a(), nb, f2.c())})[0];
        }
        void nudupl(QFI &r, const QFI &f) const { r = cs_->compose_forms({f}, {f})[0]; }
        void nupow(QFI &r, const QFI &f, const Mpz &n) const { r = cs_->pow_forms({f}, {n})[0]; }
        std::vector<QFI> nucomp(const std::vector<QFI> &f1, const std::vector<QFI> &f2) const { return cs_->compose_forms(f1, f2); }
        std::vector<QFI> nupow(const std::vector<QFI> &f, const std::vector<Mpz> &n) const { return cs_->pow_forms(f, n); }

      private:
        const HIPCryptoSystem *cs_;
    };
    class Hsm2kHandle {
      public:
        explicit Hsm2kHandle(const HIPCryptoSystem *cs) : cs_(cs) {}
        ClassGroupHandle Cl_G() const { return ClassGroupHandle(cs_); }
        ClassGroupHandle Cl_Delta() const { return ClassGroupHandle(cs_); }
        uint32_t k() const { return cs_->k_; }
        bool compact_variant() const { return false; }
        Mpz cleartext_bound() const {
            Mpz m;
            mpz_setbit(m.get(), cs_->k_);
            return m;
        }
        const Mpz &encrypt_randomness_bound() const { return cs_->exponent_bound_; }
        const QFI &h() const { return cs_->h_; }

      private:
        const HIPCryptoSystem *cs_;
    };
    Hsm2kHandle get_hsm2k() const { return Hsm2kHandle(this); }

    // ---- binary format of a plaintext tensor (reference: cpu_cryptosystem.inl:229-318): u32 ndim; u32 shape[];
    // u64 off[E] (bit 63: sgn != 1); little-endian magnitudes in slots of bits/8 + 1 bytes
    String serialize_plaintext_tensor(const Tensor<PlainText *> &t) const {
        const uint32_t ndim = (uint32_t)t.ndim();
        const size_t E = t.num_elements();
        std::vector<uint64_t> offs(E);
        uint64_t last = 0;
        for (size_t i = 0; i < E; i++) {
            offs[i] = last | (t[i]->sgn() != 1 ? (1ull << 63) : 0ull);
            last += mpz_sizeinbase(t[i]->get(), 2) / 8 + 1;
        }
        String data(4 + 4 * (size_t)ndim + 8 * E + last, '\0');
        char *p = &data[0];
        memcpy(p, &ndim, 4);
        p += 4;
        for (uint32_t i = 0; i < ndim; i++) {
            const uint32_t dim = (uint32_t)t.shape()[i];
            memcpy(p, &dim, 4);
            p += 4;
        }
        if (E) memcpy(p, offs.data(), 8 * E);
        p += 8 * E;
        for (size_t i = 0; i < E; i++) mpz_export(p + (offs[i] & ~(1ull << 63)), nullptr, -1, 1, -1, 0, t[i]->get());
        return data;
    }
    Tensor<PlainText *> deserialize_plaintext_tensor(const String &data) const {
        if (data.size() < 4) throw std::invalid_argument("tensor buffer too short");
        uint32_t ndim;
        memcpy(&ndim, data.data(), 4);
        if (ndim > 8 || data.size() < 4 + 4 * (size_t)ndim) throw std::invalid_argument("tensor buffer too short");
        std::vector<size_t> shape(ndim);
        uint64_t E = 1;
        for (uint32_t i = 0; i < ndim; i++) {
            uint32_t dim;
            memcpy(&dim, data.data() + 4 + 4 * i, 4);
            if (dim != 0 && E > (1ull << 40) / dim) throw std::invalid_argument("tensor too large");
            E *= dim;
            shape[i] = dim;
        }
        const size_t hdr = 4 + 4 * (size_t)ndim + 8 * E;
        if (data.size() < hdr) throw std::invalid_argument("tensor buffer too short");
        const uint64_t M = ~(1ull << 63);
        const char *tab = data.data() + 4 + 4 * ndim, *body = data.data() + hdr;
        const uint64_t blen = data.size() - hdr;
        Tensor<PlainText *> out = ndim ? Tensor<PlainText *>(shape, nullptr) : Tensor<PlainText *>((PlainText *)nullptr);
        Tensor<PlainText *> flat = out;
        if (ndim) flat.flatten();
        for (uint64_t i = 0; i < E; i++) {
            uint64_t o, o2;
            memcpy(&o, tab + 8 * i, 8);
            if (i + 1 < E) {
                memcpy(&o2, tab + 8 * (i + 1), 8);
                o2 &= M;
            } else {
                o2 = blen;
            }
            const uint64_t st = o & M;
            if (o2 < st || o2 > blen) throw std::invalid_argument("corrupt offset table");
            Mpz v;
            mpz_import(v.get(), o2 - st, -1, 1, -1, 0, body + st);
            if (o >> 63) v.neg();
            flat[i] = new PlainText(std::move(v));
        }
        return out;
    }

  private:
    static constexpr size_t REC = 168, REC_A = 0, REC_B = 40, REC_C = 80, REC_SIGN = 160, EXPW = 32;
    static std::vector<std::string> first_tokens(const String &data, size_t n) {
        std::istringstream ss(data);
        std::vector<std::string> t(n);
        for (size_t i = 0; i < n; i++)
            if (!(ss >> t[i])) throw std::invalid_argument("malformed text value");
        return t;
    }
    static Mpz parse_mpz(const std::string &tok) {
        Mpz v;
        if (mpz_set_str(v.get(), tok.c_str(), 10) != 0) throw std::invalid_argument("malformed integer");
        return v;
    }
    static String form_text(const QFI &f) { return f.a().str() + " " + f.b().str() + " " + f.c().str(); }
    static QFI form_from(const std::vector<std::string> &t, size_t i) { return QFI(parse_mpz(t[i]), parse_mpz(t[i + 1]), parse_mpz(t[i + 2])); }
    // (c1 h^r, c2 pk^r) with a fresh r: composing with an encryption of zero
    CipherText rerandomized(const PublicKey &pk, const CipherText &ct) const {
        if (!rerandomize_) return ct;
        const CipherText z = encrypt(pk, Mpz(0ul));
        std::vector<QFI> r = compose_forms({ct.c1(), ct.c2()}, {z.c1(), z.c2()});
        return CipherText(r[0], r[1]);
    }
    bool rerandomize_ = true;
    bool resident_gather_ = true;                          // upload(): elements of resident blocks are gathered on the device
    std::shared_ptr<std::atomic<uint64_t>> downloads_ = std::make_shared<std::atomic<uint64_t>>(0);
    TensorRandomness tensor_randomness_ = TensorRandomness::None;
    // n exponent records of r_i, uniform below exponent_bound
    std::vector<uint32_t> draw_randomness(size_t n) const {
        std::vector<uint32_t> ex(n * EXPW, 0);
        Mpz r;
        std::lock_guard<std::mutex> lk(rng_mutex_);
        for (size_t i = 0; i < n; i++) {
            mpz_urandomm(r.get(), rng_, exponent_bound_.get());
            pack_exponent(r, &ex[i * EXPW]);
        }
        return ex;
    }
    void rerandomize_into(const PublicKey &pk, const DeviceTensor &in, DeviceTensor &out) const {
        if (in.n_ == 0) return;
        Staged dr = stage(draw_randomness(in.n_));
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        check(cofhe_hip_rerandomize_records(ctx_, in.ptr_, dr.ptr, h_rec_.data(), pkrec.data(), out.ptr_, in.n_, nullptr));
    }
    // a result of this object (its own block, nobody else's view) re-randomised in place in PerElement mode
    void rerandomize_result(const PublicKey &pk, DeviceTensor &t) const {
        if (tensor_randomness_ == TensorRandomness::PerElement) rerandomize_into(pk, t, t);
    }
    // mode 0: ct + pt, 1: ct - pt, 2: pt - ct (cofhe_hip_add_plain_records); 0-D in, 0-D out
    Tensor<CipherText *> plaintext_addend(const PublicKey &pk, const Tensor<CipherText *> &ct, const Tensor<PlainText *> &pt, int mode) const {
        if (ct.is_zero_degree() && pt.is_zero_degree()) {
            Tensor<CipherText *> r = plaintext_addend(pk, Tensor<CipherText *>(1, ct.get_value()), Tensor<PlainText *>(1, pt.get_value()), mode);
            return Tensor<CipherText *>(r.at(0));
        }
        if (ct.is_zero_degree() != pt.is_zero_degree() || ct.shape() != pt.shape()) throw std::invalid_argument("Tensor shapes must be equal");
        const size_t E = ct.num_elements();
        const bool fresh = tensor_randomness_ == TensorRandomness::PerElement;
        // without fresh randomness there is no block of r (a null pointer) and the records of h and pk are not read
        Staged dpl = stage(pack_exponents(pt)), dr = fresh && E ? stage(draw_randomness(E)) : Staged();
        const std::array<uint32_t, REC> pkrec = dr.ptr ? record_of(pk) : std::array<uint32_t, REC>{};
        DeviceTensor in = upload(ct);
        DeviceTensor out = alloc(ct.shape(), E);
        check(cofhe_hip_add_plain_records(ctx_, in.ptr_, dpl.ptr, dr.ptr, h_rec_.data(), pkrec.data(), f_rec_.data(), out.ptr_, E, k_, mode, nullptr));
        return download(std::move(out));
    }
    Tensor<CipherText *> encrypt_tensor_fresh(const PublicKey &pk, const Tensor<PlainText *> &pts) const {
        const size_t E = pts.num_elements();
        Staged dr = stage(draw_randomness(E)), dpl = stage(pack_exponents(pts));
        const std::array<uint32_t, REC> pkrec = record_of(pk);
        DeviceTensor out = alloc(shape_of(pts), E);
        check(cofhe_hip_encrypt_fresh_records(ctx_, dpl.ptr, dr.ptr, h_rec_.data(), pkrec.data(), f_rec_.data(), out.ptr_, E, k_, nullptr));
        return download(std::move(out));
    }

    // ---- staging: what every member that reaches the device is made of ---------------------------------------------------------
    // A device block together with the host words copied into it.  cofhe_hip_upload is an asynchronous copy from pageable memory,
    // so the words must outlive it: the destructor waits for the stream the copy (and the kernels that read the block) ran on and
    // only then frees the block and lets the words go.  An error of that wait surfaces at the next call that checks the stream --
    // the download of the records, at the latest.  Without words (device_buffer) it is a block the device writes and a download
    // reads: there is no host memory to protect, the free is ordered on the stream like every free of the block cache, no wait.
    struct Staged {
        cofhe_hip_ctx *ctx = nullptr;
        void *ptr = nullptr;
        std::vector<uint32_t> words;
        Staged() = default;
        Staged(Staged &&o) noexcept : ctx(o.ctx), ptr(o.ptr), words(std::move(o.words)) { o.ptr = nullptr; }      // the words keep their address
        Staged(const Staged &) = delete;
        Staged &operator=(const Staged &) = delete;
        ~Staged() {
            if (!ptr) return;
            if (!words.empty()) cofhe_hip_stream_sync(ctx, nullptr);
            cofhe_hip_free(ctx, ptr);
        }
    };
    Staged device_buffer(size_t bytes) const {
        Staged s;
        s.ctx = ctx_;
        check(cofhe_hip_malloc(ctx_, bytes, &s.ptr));          // 0 bytes give a block of 4
        return s;
    }
    Staged stage(std::vector<uint32_t> &&words) const {
        Staged s = device_buffer(words.size() * 4);
        s.words = std::move(words);
        check(cofhe_hip_upload(ctx_, s.ptr, s.words.data(), s.words.size() * 4, nullptr));
        return s;
    }
    // records from the host into a tensor's own block; waits for the copy, so `recs` may go when this returns
    void fill(DeviceTensor &d, const std::vector<uint32_t> &recs) const {
        check(cofhe_hip_upload(ctx_, d.ptr_, recs.data(), recs.size() * 4, nullptr));
        synchronize();
    }
    // the shape of a result of t's: a 0-D tensor gives one element
    template <typename T>
    static std::vector<size_t> shape_of(const Tensor<T> &t) { return t.is_zero_degree() ? std::vector<size_t>{1} : t.shape(); }
    // the element of a one-element result tensor, by value; the heap object goes
    template <typename T>
    static T single(const Tensor<T *> &r) {
        T out = *r.at(0);
        delete r.at(0);
        return out;
    }
    // the uploaded one-element tensor a product starts from: `zero`, or a fresh encryption of zero
    DeviceTensor zero_tensor(const PublicKey &pk, const CipherText *zero) const {
        CipherText z = zero ? *zero : encrypt(pk, make_plaintext(0));
        return upload(Tensor<CipherText *>(1, &z));
    }
    // n plaintexts of `words` words each, read from the device into a tensor of `shape`: the magnitude is the words below the top
    // one; the top word is the sign when sign_word is set and ignored otherwise.  not_in_f, given for values that kernels read
    // off ciphertext records (the two decryptions), is thrown for a top word that is not 0, after the device status word has
    // had its say.
    Tensor<PlainText *> read_plaintexts(const void *d, size_t n, size_t words, const std::vector<size_t> &shape, bool sign_word,
                                        const char *not_in_f = nullptr) const {
        std::vector<uint32_t> w(n * words);
        check(cofhe_hip_download(ctx_, w.data(), d, w.size() * 4, nullptr));
        if (not_in_f) DeviceBlock::throw_on_device_status(ctx_);
        Tensor<PlainText *> out(shape, nullptr);
        for (size_t i = 0; i < n; i++) {
            const uint32_t top = w[i * words + words - 1];
            if (not_in_f && top != 0) throw std::runtime_error(not_in_f);
            Mpz v;
            mpz_import(v.get(), words - 1, -1, 4, 0, 0, &w[i * words]);
            if (sign_word && top) v.neg();
            out[i] = new PlainText(std::move(v));
        }
        return out;
    }
    // n form records read from the device, never with a cap bit set in the status word
    std::vector<QFI> read_forms(const void *d, size_t n) const {
        std::vector<uint32_t> recs(n * REC);
        check(cofhe_hip_download(ctx_, recs.data(), d, recs.size() * 4, nullptr));
        DeviceBlock::throw_on_device_status(ctx_);
        std::vector<QFI> out(n);
        COFHE_HOST_PARALLEL_FOR
        for (size_t i = 0; i < n; i++) out[i] = unpack_form(&recs[i * REC]);
        return out;
    }
    // b of a lookup table of `size` entries, n_tab of them for n elements: size = 2^b, 1 <= b <= COFHE_HIP_LUT_MAX_BITS, b <= k
    uint32_t lut_bits(size_t size, size_t n_tab, size_t n) const {
        uint32_t b = 0;
        while (b <= COFHE_HIP_LUT_MAX_BITS && ((size_t)1 << b) != size) b++;
        if (b == 0 || b > COFHE_HIP_LUT_MAX_BITS || b > k_) throw std::invalid_argument("lookup table: 2^b entries, 1 <= b <= 12, b <= k");
        if (n_tab == 0 || n % n_tab != 0) throw std::invalid_argument("lookup tables: their count must divide the element count");
        return b;
    }
    static void check(int rc) {
        if (rc == COFHE_HIP_OK) return;
        std::string msg = cofhe_hip_last_error();
        if (rc == COFHE_HIP_ESHAPE || rc == COFHE_HIP_ENDIM || rc == COFHE_HIP_EINVAL) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
    // the 14 extents of a convolution's geometry, each within 32 bits
    static cofhe_hip_conv2d_geometry conv_geometry(const std::array<size_t, 14> &v) {
        uint32_t u[14];
        for (size_t i = 0; i < 14; i++) {
            if (v[i] > 0xFFFFFFFFull) throw std::invalid_argument("convolution geometry: extent out of range");
            u[i] = (uint32_t)v[i];
        }
        return cofhe_hip_conv2d_geometry{u[0], u[1], u[2], u[3], u[4], u[5], u[6], u[7], u[8], u[9], u[10], u[11], u[12], u[13]};
    }
    static bool try_put(const Mpz &v, uint32_t *dst, size_t words) {
        if (v.nbits() > words * 32) return false;
        size_t cnt = 0;
        mpz_export(dst, &cnt, -1, 4, 0, 0, v.get());
        return true;
    }
    // false when a coefficient exceeds its limb plane (no exception: called inside OpenMP loops)
    static bool try_pack_form(const QFI &f, uint32_t *rec) {
        const bool ok = try_put(f.a(), rec + REC_A, 40) && try_put(f.b(), rec + REC_B, 40) && try_put(f.c(), rec + REC_C, 80);
        rec[REC_SIGN] = f.b().sgn() < 0 ? 1u : 0u;
        return ok;
    }
    static void pack_form(const QFI &f, uint32_t *rec) {
        if (!try_pack_form(f, rec)) throw std::invalid_argument("form coefficient outside the supported range");
    }
    // packs n forms fetched by get(i) into consecutive records, in parallel
    template <typename Get>
    static void pack_forms(size_t n, uint32_t *recs, Get get) {
        std::atomic<bool> bad{false};
        COFHE_HOST_PARALLEL_FOR
        for (size_t i = 0; i < n; i++)
            if (!try_pack_form(get(i), recs + i * REC)) bad = true;
        if (bad) throw std::invalid_argument("form coefficient outside the supported range");
    }
    static QFI unpack_form(const uint32_t *rec) {
        Mpz a, b, c;
        mpz_import(a.get(), 40, -1, 4, 0, 0, rec + REC_A);
        mpz_import(b.get(), 40, -1, 4, 0, 0, rec + REC_B);
        mpz_import(c.get(), 80, -1, 4, 0, 0, rec + REC_C);
        if (rec[REC_SIGN]) b.neg();
        return QFI(std::move(a), std::move(b), std::move(c));
    }
    static void pack_exponent(const Mpz &e, uint32_t *rec) {
        if (e.nbits() > 31 * 32) throw std::invalid_argument("exponent wider than 992 bits");
        size_t cnt = 0;
        mpz_export(rec, &cnt, -1, 4, 0, 0, e.get());
        rec[31] = e.sgn() < 0 ? 1u : 0u;
    }
    static std::vector<uint32_t> exponent_record(const Mpz &e) {
        std::vector<uint32_t> ex(EXPW, 0);
        pack_exponent(e, ex.data());
        return ex;
    }
    // the elements of s in row-major order, whatever its shape, into consecutive (zeroed) exponent records
    static void pack_exponents(const Tensor<PlainText *> &s, uint32_t *recs) {
        for (size_t i = 0; i < s.num_elements(); i++) pack_exponent(*s[i], recs + i * EXPW);
    }
    static std::vector<uint32_t> pack_exponents(const Tensor<PlainText *> &s) {
        std::vector<uint32_t> ex(s.num_elements() * EXPW, 0);
        pack_exponents(s, ex.data());
        return ex;
    }
    static std::array<uint32_t, REC> record_of(const QFI &f) {
        std::array<uint32_t, REC> rec{};
        pack_form(f, rec.data());
        return rec;
    }
    DeviceTensor alloc(const std::vector<size_t> &shape, size_t n) const {
        DeviceTensor d;
        d.ctx_ = ctx_;
        d.shape_ = shape;
        d.n_ = n;
        check(cofhe_hip_malloc(ctx_, n * 2 * REC * 4, &d.ptr_));
        return d;
    }
    static std::vector<size_t> extents(const uint64_t *e, uint32_t nd) { return std::vector<size_t>(e, e + nd); }
    static std::vector<uint64_t> shape64(const DeviceTensor &x) { return std::vector<uint64_t>(x.shape_.begin(), x.shape_.end()); }
    // one view call: the box of `view`, whose source is x, into the resident tensor `out`, whose shape is the view's destination
    void view_into(const DeviceTensor &x, const cofhe_hip_view &view, const DeviceTensor *fill, DeviceTensor &out) const {
        if (view.src_ndim > COFHE_HIP_VIEW_MAX_DIMS || extents(view.src_extent, view.src_ndim) != x.shape_)
            throw std::invalid_argument("view: the descriptor's source is not the tensor's shape");
        if (fill && fill->n_ != 1) throw std::invalid_argument("view: the fill is one element");
        check(cofhe_hip_view_records(ctx_, &view, x.ptr_, fill ? fill->ptr_ : nullptr, out.ptr_, 2 * REC, nullptr));
    }
    // d tensors of E ciphertexts each as ONE device tensor [d, E], tensor-major: the layout of the bases of
    // cofhe_hip_pow_dot_records.  The records of a resident tensor are taken from its block, not rebuilt from GMP integers.
    DeviceTensor stack(const Vector<Tensor<CipherText *>> &ts) const {
        const size_t d = ts.size(), E = d ? ts[0].num_elements() : 0;
        std::vector<uint32_t> recs(d * E * 2 * REC, 0);
        for (size_t i = 0; i < d; i++) {
            if (ts[i].num_elements() != E) throw std::invalid_argument("Tensor shapes must be equal");
            uint32_t *dst = &recs[i * E * 2 * REC];
            const Tensor<CipherText *> &t = ts[i];
            std::shared_ptr<DeviceBlock> b = whole_block(t);
            if (b && b->ctx == ctx_)
                std::memcpy(dst, b->records(), E * 2 * REC * 4);
            else
                pack_forms(2 * E, dst, [&](size_t r) -> const QFI & { const CipherText &c = *t[r >> 1]; return (r & 1) ? c.c2() : c.c1(); });
        }
        DeviceTensor out = alloc({d, E}, d * E);
        fill(out, recs);
        return out;
    }

    Tensor<PlainText *> plaintext_tensor_op(const Tensor<PlainText *> &a, const Tensor<PlainText *> &b, bool mul) const {
        if (a.is_zero_degree() && b.is_zero_degree())
            return Tensor<PlainText *>(new PlainText(mul ? multiply_plaintexts(*a.get_value(), *b.get_value())
                                                         : add_plaintexts(*a.get_value(), *b.get_value())));
        if (a.shape() != b.shape()) throw std::invalid_argument("Tensor shapes must be equal");
        if (a.ndim() != 1) throw std::runtime_error("Not implemented");
        Tensor<PlainText *> res(a.shape(), nullptr);
        for (size_t i = 0; i < a.num_elements(); i++)
            res[i] = new PlainText(mul ? multiply_plaintexts(*a[i], *b[i]) : add_plaintexts(*a[i], *b[i]));
        return res;
    }

    // Distribution matrix of the t-out-of-n access structure: OR over the C(n,t) threshold sets of
    // the AND of t parties (what compute_M_AND / compute_M_OR build recursively,
    // cpu_cryptosystem_distributed.inl:22-127), written in closed form: column 0 carries the secret;
    // set i owns rows i*t .. i*t+t-1 and columns 1+i*(t-1) .. (i+1)*(t-1); its first row is all
    // ones over column 0 and its own columns, its row r >= 1 is the unit vector of its column t-r.
    static std::vector<std::vector<int>> distribution_matrix(size_t n, size_t t) {
        if (t == 0 || t > n) throw std::invalid_argument("threshold must be between 1 and the number of parties");
        size_t sets = 1;
        for (size_t i = 1; i <= t; i++) sets = sets * (n - t + i) / i;
        const size_t cols = 1 + sets * (t - 1);
        std::vector<std::vector<int>> M(sets * t, std::vector<int>(cols, 0));
        for (size_t i = 0; i < sets; i++) {
            const size_t c0 = 1 + i * (t - 1);
            M[i * t][0] = 1;
            for (size_t j = 0; j + 1 < t; j++) M[i * t][c0 + j] = 1;
            for (size_t r = 1; r < t; r++) M[i * t + r][c0 + (t - r) - 1] = 1;
        }
        return M;
    }

    // ---- setup (host; literature restatement) ----------------------------------
    static uint32_t disc_bits(uint32_t sec) {
        switch (sec) {
            case 112: return 1348;
            case 128: return 1827;
            case 192: return 3598;
            case 256: return 5971;
            default: throw std::invalid_argument("unsupported security level");
        }
    }
    void random_prime(Mpz &p, uint32_t bits, unsigned long mod8) {
        do {
            mpz_urandomb(p.get(), rng_, bits);
            mpz_setbit(p.get(), bits - 1);
            unsigned long r = mpz_fdiv_ui(p.get(), 8);
            mpz_sub_ui(p.get(), p.get(), r);
            mpz_add_ui(p.get(), p.get(), mod8);
        } while (mpz_sizeinbase(p.get(), 2) != bits || !mpz_probab_prime_p(p.get(), 30));
    }
    void generate_parameters() {
        const uint32_t nb = disc_bits(sec_level_);
        Mpz p, q;
        do {
            random_prime(p, nb / 2, 3);
            random_prime(q, nb - nb / 2, 5);
            mpz_mul(N_.get(), p.get(), q.get());
        } while (mpz_sizeinbase(N_.get(), 2) != nb || mpz_jacobi(p.get(), q.get()) != -1);
        derive_from_N();
    }
    void derive_from_N() {
        mpz_mul_ui(deltaK_.get(), N_.get(), 8);
        deltaK_.neg();
        mpz_mul_2exp(delta_.get(), deltaK_.get(), 2 * (k_ + 1));
        Mpz a, b, c;
        mpz_setbit(a.get(), 2 * k_);
        mpz_setbit(b.get(), k_ + 1);
        mpz_ui_sub(c.get(), 1, deltaK_.get());
        f_ = QFI(a, b, c);
        mpz_setbit(exponent_bound_.get(), (mpz_sizeinbase(deltaK_.get(), 2) + 1) / 2 + 11 + 40);
    }
    void open_device() {
        Mpz ad = delta_;
        ad.neg();
        std::vector<uint8_t> bytes((mpz_sizeinbase(ad.get(), 2) + 7) / 8 + 1, 0);
        size_t cnt = 0;
        mpz_export(bytes.data(), &cnt, -1, 1, 0, 0, ad.get());
        check(cofhe_hip_ctx_create(device_, bytes.data(), cnt, &ctx_));
        ctx_owner_ = std::shared_ptr<cofhe_hip_ctx>(ctx_, [](cofhe_hip_ctx *p) { cofhe_hip_ctx_destroy(p); });
    }
    void compute_generator() {
        // h = (t^2)^(2^k), t the prime form of the smallest odd prime l with (Delta / l) = 1
        unsigned long l = 3;
        Mpz L;
        for (;; l += 2) {
            mpz_set_ui(L.get(), l);
            if (mpz_probab_prime_p(L.get(), 20) && mpz_kronecker_ui(delta_.get(), l) == 1) break;
        }
        unsigned long dm = mpz_fdiv_ui(delta_.get(), 4 * l);
        unsigned long bb = 0;
        for (unsigned long b = 0; b <= l; b++)
            if ((b * b) % (4 * l) == dm) { bb = b; break; }
        Mpz a(l), b(bb), c;
        mpz_mul(c.get(), b.get(), b.get());
        mpz_sub(c.get(), c.get(), delta_.get());
        mpz_divexact_ui(c.get(), c.get(), 4 * l);
        Mpz e;
        mpz_setbit(e.get(), k_ + 1);
        h_ = pow_forms({QFI(a, b, c)}, {e})[0];
    }
    // the records of f and h, packed once where both are known; nothing writes them after construction (threads share the object)
    void pack_generators() {
        f_rec_ = record_of(f_);
        h_rec_ = record_of(h_);
    }
    void init_mpf() {
        mpf_init(scaling_factor_); mpf_init(mM_); mpf_init(mM_half_);
        mpf_set_d(scaling_factor_, 2); mpf_set_d(mM_, 2);
        mpf_pow_ui(scaling_factor_, scaling_factor_, 0);
        mpf_pow_ui(mM_, mM_, k_);
        mpf_div_ui(mM_half_, mM_, 2);
    }

    uint32_t sec_level_, k_;
    int device_;
    Mpz N_, deltaK_, delta_;
    QFI f_, h_;
    std::array<uint32_t, REC> f_rec_{}, h_rec_{};
    Mpz exponent_bound_;
    cofhe_hip_ctx *ctx_ = nullptr;
    std::shared_ptr<cofhe_hip_ctx> ctx_owner_;
    mutable gmp_randstate_t rng_;
    mutable std::mutex rng_mutex_;
    mpf_t scaling_factor_, mM_, mM_half_;
};

// factory with the reference's signature (include/cofhe.hpp:96-99); Device::GPU is the only
// device this engine serves -- there is no CPU path to fall back to.
inline HIPCryptoSystem make_cryptosystem(uint32_t security_level, uint32_t k, Device device) {
    if (device != Device::GPU) throw std::invalid_argument("cofhe_amd serves Device::GPU only");
    return HIPCryptoSystem(security_level, k);
}
// the two enum overloads (include/cofhe.hpp:102-121).  LOW maps to 112 here: the parameter table of the scheme has no
// 80-bit row (the reference passes 80 on to BICYCL).  The third overload derives k from the precision and the
// multiplicative depth -- the reference computes that k and then passes `depth` instead (cofhe.hpp:111-120); the
// computed k is what is used here.
inline uint32_t security_bits(SecurityLevel l) { return l == SecurityLevel::LOW ? 112u : l == SecurityLevel::MEDIUM ? 128u : 256u; }
inline HIPCryptoSystem make_cryptosystem(SecurityLevel security_level, uint32_t k, Device device) {
    return make_cryptosystem(security_bits(security_level), k, device);
}
inline HIPCryptoSystem make_cryptosystem(SecurityLevel security_level, Precision precision, uint32_t depth, Device device) {
    const uint32_t k = depth * (precision == Precision::FP32 ? 64u : 128u);
    return make_cryptosystem(security_bits(security_level), k, device);
}

}  // namespace CoFHE
