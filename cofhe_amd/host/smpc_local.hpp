// smpc_local.hpp -- the LOCAL part of CoFHE's ciphertext x ciphertext multiplication (Beaver
// triplets) on the MI355X engine.
//
// Reference: SMPCCipherTextMultiplier<CryptoSystem> (include/smpc/ciphertext_multiplications.hpp:8-175)
// runs every tensor operation of the protocol on the caller's CryptoSystem and reaches the
// network only through its SMPCClient for two things: get_beavers_triplets(n) and
// decrypt_tensor(ct) (threshold decryption by the CoFHE nodes).  Here that client is a template
// parameter; LocalSMPCClient below answers both calls in-process (triplets from fresh
// randomness, decryption either with the secret key or by t-of-n threshold decryption:
// part_decrypt_tensor per party + combine_part_decryption_results_tensor), so the whole
// multiplication is the sequence of GPU kernels the networked system would run, minus sockets.
// The protocol per element (ciphertext_multiplications.hpp:115-160), with (a, b, c = ab) a triplet:
//   e = Dec(x - a), d = Dec(y - b);  x*y = e*b + d*a + c + e*d
// i.e. 2 negations, 5 additions, 2 scalings, 1 encryption and 2 decryptions per product.
// LocalCipherTextMultiplier::set_direct_differences(true) opens x - a, y - b with sub_ciphertext_tensors (one composition
// per record where a negation is ct^(2^k - 1): k squarings and a product) and closes with add_plaintext_tensor(..., e*d)
// (c2 o f^(ed) against the cached table of f) instead of an encryption and an addition: no negation and no encryption.
//
// Matrix triplets (set_matrix_triplets(true), the 2-D product only; the reference has no such flow).  The reference expands an
// n x m by m x p product into n m p element products: n m p triplets and 2 n m p threshold decryptions.  With ONE matrix
// triplet [A] (n x m), [B] (m x p), [C] = [A B]:
//   E = Dec(X - A), D = Dec(Y - B);  X Y = E [B] + [A] D + [C] + E D
// which opens n m + m p values, and spends a plaintext-left product (matmul_plaintext_ciphertext_tensors), a ciphertext-left
// product (scal_ciphertext_tensors) and a plaintext matrix product mod 2^k (matmul_plaintext_tensors).
//
// Convolution triplets (conv2d_ciphertext_tensors: an encrypted image under encrypted filters; the reference has no convolution).
// Convolution is bilinear, so the identity above holds with * for the product:  [A] image-shaped, [Bf] filter-shaped,
// [C] = [A * Bf];  E = Dec(X - A), D = Dec(Wf - Bf);  X * Wf = E * [Bf] + [A] * D + [C] + E * D -- B H W C + kh kw C Co opened
// values, every pixel once, where a matrix triplet on the patch matrix opens each pixel kh kw times.
//
// Polynomials (evaluate_polynomial_ciphertext_tensor, square_ciphertext_tensor; the reference has no such flow).  A degree-d
// polynomial with plaintext coefficients by chained products opens 2 (d - 1) values per element in d - 1 rounds.  With a power
// tuple ([a], .., [a^d]) per element:  e = Dec(x - a);  [p(x)] = prod_i [a^i]^(q_i(e)) o f^(q_0(e)),  q the Taylor shift of p at
// e mod 2^k -- one opened value and one round whatever d (poly_close_ciphertext_tensor, on the device from end to end).
//
// Division by public divisors (divide_ciphertext_tensor_by_plaintext, truncate_ciphertext_tensor, avg_pool2d_ciphertext_tensor;
// the reference's ComputeOperation::DIVIDE answers "Not implemented").  With a division pair ([r], [r_q]), r_q = floor(s(r) / D),
// per element:  e = Dec(x - r);  [y] = [r_q] o f^(floor(s(e) / D)),  s the centred residue mod 2^k -- one opened value, no
// encryption, no ladder; y is floor(x / D) or one less unless s(r) + s(e) wraps (probability |x| / 2^k per element).
//
// Exact division and remainders by small divisors (divide_exact_ciphertext_tensor_by_plaintext, truncate_exact_ciphertext_tensor,
// remainder_ciphertext_tensor, decompose_ciphertext_tensor, avg_pool2d_exact_ciphertext_tensor).  With an exact-division tuple
// ([r], [T_0], .., [T_{D-1}]), T_j = floor(s(r) / D) + [s(r) mod D + j >= D], per element:  e = Dec(x - r);  [y] = [T_{s(e) mod D}]
// o f^(floor(s(e) / D)) -- one opened value, one round, y = floor(x / D) EXACTLY unless s(r) + s(e) wraps; D <= 4096 per round,
// D fresh encryptions per element.  Every [T_j] carries its own randomness whatever the randomness mode.
//
// Table lookups (lookup_ciphertext_tensor, relu_ciphertext_tensor, max_ciphertext_tensors, max_pool2d_ciphertext_tensor; the
// reference has no comparison).  With a lookup tuple ([r], [T_0], .., [T_{2^b - 1}]), T_j = g[(j + r) mod 2^b], per element:
// e = Dec(x - r);  [y] = [T_{e mod 2^b}] -- one opened value, one round, y = g[x mod 2^b] exactly for ANY public table g of 2^b
// plaintexts, and the closing step is a copy.  Every [T_j] carries its own randomness whatever the randomness mode.
//
// Piecewise-polynomial activations (evaluate_spline_ciphertext_tensor: sigmoid, tanh, GELU, exp, 1/x as splines; the reference
// has none).  With a spline tuple ([r], [q_{j,i}], j < 2^b, i <= d), q_{j,.} the Taylor shift of piece (j + seg(r)) mod 2^b at r
// minus the piece's origin, per element:  e = Dec(x - r);  j = seg(e);  [y] = [q_{j,0}] o prod_{i=1..d} [q_{j,i}]^(e^i) -- one
// opened value, one round, 2^b (d + 1) ciphertexts per element for a (t + b)-bit window; y is the value at x of the element's
// own piece or of the piece below (the carry of the low t bits is lost), so a piece serves two segments.
//
// Sign, ReLU and max on windows of up to 64 bits (is_nonnegative_ciphertext_tensor, relu_wide_ciphertext_tensor,
// max_wide_ciphertext_tensors; the reference has no comparison).  With a comparison tuple ([r], [T]), T[j][c] = 2^j sgn(r_j - c)
// over the n = ceil(bits / d) digits of r mod 2^bits:  e = Dec(x - r) names two thresholds A, B with [x < 0] = [r >= A] - [r >= B]
// + [A > B];  [S_t] = prod_j [T[j][t_j]] has the sign of r - t;  one lookup of n + 1 bits over [S_A], [S_B] closes it -- two
// rounds, three opened values per element, n 2^d + 2^(n+2) ciphertexts per element where a lookup takes 2^bits; exact.
#pragma once
#include "hip_cryptosystem.hpp"

namespace CoFHE {

// What the multiplier needs from "the network".  Mirrors the members of SMPCClient it calls
// (include/smpc/smpc_client.hpp: crypto_system(), network_public_key(), get_beavers_triplets,
// decrypt, decrypt_tensor).
template <typename CryptoSystem>
class LocalSMPCClient {
  public:
    using SecretKey = typename CryptoSystem::SecretKey;
    using SecretKeyShare = typename CryptoSystem::SecretKeyShare;
    using PublicKey = typename CryptoSystem::PublicKey;
    using PlainText = typename CryptoSystem::PlainText;
    using CipherText = typename CryptoSystem::CipherText;
    using PartDecryptionResult = typename CryptoSystem::PartDecryptionResult;

    // single key holder
    LocalSMPCClient(CryptoSystem &cs, const SecretKey &sk) : cs_(cs), sk_(sk), pk_(cs.keygen(sk)) {}
    // t-of-n: decryption goes through the threshold path with the first threshold set {0..t-1}
    LocalSMPCClient(CryptoSystem &cs, const SecretKey &sk, size_t threshold, size_t parties)
        : cs_(cs), sk_(sk), pk_(cs.keygen(sk)), threshold_(threshold) {
        auto shares = cs.keygen(sk, threshold, parties);
        for (size_t j = 0; j < threshold; j++) shares_.push_back(shares[j][0]);
    }

    CryptoSystem &crypto_system() { return cs_; }
    const PublicKey &network_public_key() const { return pk_; }

    // n x 3 tensor of (Enc a, Enc b, Enc ab), a and b uniform in the message space Z/2^k (the
    // reference's generator, include/smpc/beavers_triplet_generation.hpp, is a network protocol
    // between the nodes)
    Tensor<CipherText *> get_beavers_triplets(size_t n) {
        Tensor<PlainText *> pa(n, nullptr), pb(n, nullptr);
        for (size_t i = 0; i < n; i++) {
            pa[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
            pb[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        }
        auto pc = cs_.multiply_plaintext_tensors(pa, pb);
        auto ea = cs_.encrypt_tensor(pk_, pa), eb = cs_.encrypt_tensor(pk_, pb), ec = cs_.encrypt_tensor(pk_, pc);
        Tensor<CipherText *> t(n, 3, nullptr);
        for (size_t i = 0; i < n; i++) {
            t.at(i, 0) = ea[i];
            t.at(i, 1) = eb[i];
            t.at(i, 2) = ec[i];
            delete pa[i];
            delete pb[i];
            delete pc[i];
        }
        return t;
    }

    // one matrix triplet: {[A] (n x m), [B] (m x p), [C] = [A B mod 2^k] (n x p)}, A and B uniform in Z/2^k; the caller
    // owns the elements and uses the triplet once
    Vector<Tensor<CipherText *>> get_beavers_matrix_triplet(size_t n, size_t m, size_t p) {
        Tensor<PlainText *> pa(n, m, nullptr), pb(m, p, nullptr);
        for (size_t i = 0; i < n * m; i++) pa[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        for (size_t i = 0; i < m * p; i++) pb[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        auto pc = cs_.matmul_plaintext_tensors(pa, pb);
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor(pk_, pa));
        t.push_back(cs_.encrypt_tensor(pk_, pb));
        t.push_back(cs_.encrypt_tensor(pk_, pc));
        for (size_t i = 0; i < n * m; i++) delete pa[i];
        for (size_t i = 0; i < m * p; i++) delete pb[i];
        for (size_t i = 0; i < n * p; i++) delete pc[i];
        return t;
    }

    // one convolution triplet: {[A] (image_shape [B, H, W, C]), [Bf] (filter_shape [kh, kw, C, Co]), [C] = [A * Bf mod 2^k]
    // ([B, Ho, Wo, Co])} for the geometry given, A and Bf uniform in Z/2^k; the caller owns the elements and uses the triplet once
    Vector<Tensor<CipherText *>> get_beavers_conv2d_triplet(const std::vector<size_t> &image_shape, const std::vector<size_t> &filter_shape,
                                                            const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad,
                                                            const std::array<size_t, 2> &dilation) {
        Tensor<PlainText *> pa(image_shape, nullptr), pb(filter_shape, nullptr);
        for (size_t i = 0; i < pa.num_elements(); i++) pa[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        for (size_t i = 0; i < pb.num_elements(); i++) pb[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        auto pc = cs_.conv2d_plaintext_tensors(pa, pb, stride, pad, dilation);
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor(pk_, pa));
        t.push_back(cs_.encrypt_tensor(pk_, pb));
        t.push_back(cs_.encrypt_tensor(pk_, pc));
        for (size_t i = 0; i < pa.num_elements(); i++) delete pa[i];
        for (size_t i = 0; i < pb.num_elements(); i++) delete pb[i];
        for (size_t i = 0; i < pc.num_elements(); i++) delete pc[i];
        return t;
    }

    // power tuples for n elements: the d ciphertext tensors [a], [a^2], .., [a^d] (n elements each), a uniform in Z/2^k per
    // element and used once; the caller owns the elements.  The powers are multiply_plaintext_tensors' products, reduced mod
    // 2^k as they grow (an encryption reduces its plaintext anyway; unreduced, a^8 outgrows an exponent record).  Like the
    // triplets, the tuples of the networked system would come from a protocol between the nodes.
    Vector<Tensor<CipherText *>> get_beavers_power_tuples(size_t n, size_t d) {
        Tensor<PlainText *> pa(n, nullptr), pw(n, nullptr);
        for (size_t i = 0; i < n; i++) {
            pa[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
            pw[i] = new PlainText(*pa[i]);
        }
        Vector<Tensor<CipherText *>> t;
        for (size_t j = 1; j <= d; j++) {
            t.push_back(cs_.encrypt_tensor(pk_, pw));
            if (j == d) break;
            auto next = cs_.multiply_plaintext_tensors(pw, pa);
            for (size_t i = 0; i < n; i++) {
                mpz_fdiv_r_2exp(next[i]->get(), next[i]->get(), cs_.message_bits());
                delete pw[i];
            }
            pw = next;
        }
        for (size_t i = 0; i < n; i++) {
            delete pa[i];
            delete pw[i];
        }
        return t;
    }

    // division pairs for n elements and the public divisors div (element i takes divisor i mod count): {[r], [r_q]} with r
    // uniform in Z/2^k per element and r_q = floor(s(r) / D) mod 2^k (divide_plaintext_tensor), used once; the caller owns the
    // elements.  Like the triplets, the pairs of the networked system would come from a protocol between the nodes.
    Vector<Tensor<CipherText *>> get_division_pairs(size_t n, const Tensor<PlainText *> &div) {
        Tensor<PlainText *> pr(n, nullptr);
        for (size_t i = 0; i < n; i++) pr[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        auto prq = cs_.divide_plaintext_tensor(pr, div);
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor(pk_, pr));
        t.push_back(cs_.encrypt_tensor(pk_, prq));
        for (size_t i = 0; i < n; i++) {
            delete pr[i];
            delete prq[i];
        }
        return t;
    }

    // exact-division tuples for n elements and the small public divisors div (element i takes divisor i mod count, every one at
    // most 4096): {[r] (n elements), [T] (n rows elements, [n, rows], rows the largest divisor)} with r uniform in Z/2^k per
    // element and T[i, j] = floor(s(r_i) / D_i) + [s(r_i) mod D_i + j >= D_i], used once; the caller owns the elements.  [r] and
    // every [T_j] are encrypted with their OWN randomness whatever the randomness mode: the entries differ by 0 or 1, so entries
    // that shared c1 would give s(r) mod D, and with the opened value x mod D, away.  Like the triplets, the tuples of the
    // networked system would come from a protocol between the nodes.
    Vector<Tensor<CipherText *>> get_exact_division_tuples(size_t n, const Tensor<PlainText *> &div) {
        (void)cs_.check_small_divisors(div, n);                  // refuse before anything is drawn
        Tensor<PlainText *> pr(n, nullptr);
        for (size_t i = 0; i < n; i++) pr[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor_per_element(pk_, pr));
        t.push_back(cs_.divx_tuples_ciphertext_tensor(pk_, div, pr));
        for (size_t i = 0; i < n; i++) delete pr[i];
        return t;
    }

    // lookup tuples for n elements and the public table(s) `table` ([2^b], or [n_tab, 2^b] with element i taking table i mod
    // n_tab): {[r] (n elements), [T] (n 2^b elements, [n, 2^b])} with r uniform in Z/2^k per element and T[i, j] = table[(j +
    // r_i) mod 2^b], used once; the caller owns the elements.  [r] and every [T_j] are encrypted with their OWN randomness
    // whatever the randomness mode: entries that shared c1 would give the rotation, and with the opened value x mod 2^b, away.
    // Like the triplets, the tuples of the networked system would come from a protocol between the nodes.
    Vector<Tensor<CipherText *>> get_lookup_tuples(size_t n, const Tensor<PlainText *> &table) {
        (void)cs_.lut_table_bits(table, n);                      // refuse before anything is drawn
        Tensor<PlainText *> pr(n, nullptr);
        for (size_t i = 0; i < n; i++) pr[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor_per_element(pk_, pr));
        t.push_back(cs_.lut_tuples_ciphertext_tensor(pk_, table, pr));
        for (size_t i = 0; i < n; i++) delete pr[i];
        return t;
    }

    // spline tuples for n elements and the public spline table(s) `table` ([2^bits, d + 1], or [n_tab, 2^bits, d + 1] with
    // element i taking table i mod n_tab): {[r] (n elements), [q] (n 2^bits (d + 1) elements, [n, 2^bits, d + 1])} with r uniform
    // in Z/2^k per element and q[i, j, .] the Taylor shift of piece (j + rho_i) mod 2^bits at r_i minus the piece's origin, used
    // once; the caller owns the elements.  [r] and every [q] are encrypted with their OWN randomness whatever the randomness
    // mode, for the reason given for the lookups.  Like the triplets, the tuples of the networked system would come from a
    // protocol between the nodes.
    Vector<Tensor<CipherText *>> get_spline_tuples(size_t n, const Tensor<PlainText *> &table, uint32_t bits, uint32_t shift) {
        (void)cs_.spline_table_shape(table, n, bits, shift);     // refuse before anything is drawn
        Tensor<PlainText *> pr(n, nullptr);
        for (size_t i = 0; i < n; i++) pr[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor_per_element(pk_, pr));
        t.push_back(cs_.spline_tuples_ciphertext_tensor(pk_, table, pr, bits, shift));
        for (size_t i = 0; i < n; i++) delete pr[i];
        return t;
    }

    // comparison tuples for n elements on a window of `bits` bits in digits of digit_bits bits: {[r] (n elements), [T] (n nd 2^d
    // elements, [n, nd, 2^d], nd = ceil(bits / d))} with r uniform in Z/2^k per element and T[i, j, c] = 2^j sgn(r_ij - c), r_ij
    // digit j of r_i mod 2^bits, used once; the caller owns the elements.  [r] and every [T] are encrypted with their OWN
    // randomness whatever the randomness mode, for the reason given for the lookups.  Like the triplets, the tuples of the
    // networked system would come from a protocol between the nodes.
    Vector<Tensor<CipherText *>> get_comparison_tuples(size_t n, uint32_t bits, uint32_t digit_bits) {
        (void)cs_.cmp_shape(bits, digit_bits);                   // refuse before anything is drawn
        Tensor<PlainText *> pr(n, nullptr);
        for (size_t i = 0; i < n; i++) pr[i] = new PlainText(cs_.random_plaintext(cs_.message_bits()));
        Vector<Tensor<CipherText *>> t;
        t.push_back(cs_.encrypt_tensor_per_element(pk_, pr));
        t.push_back(cs_.cmp_tuples_ciphertext_tensor(pk_, pr, bits, digit_bits));
        for (size_t i = 0; i < n; i++) delete pr[i];
        return t;
    }

    Tensor<PlainText *> decrypt_tensor(const Tensor<CipherText *> &ct) {
        decrypted_ += ct.num_elements();
        if (threshold_ == 0) return cs_.decrypt_tensor(sk_, ct);
        Vector<Tensor<PartDecryptionResult *>> pdrs;
        for (const auto &sh : shares_) pdrs.push_back(cs_.part_decrypt_tensor(sh, ct));
        auto res = cs_.combine_part_decryption_results_tensor(ct, pdrs);
        for (auto &p : pdrs) {
            p.flatten();
            for (size_t i = 0; i < p.num_elements(); i++) delete p[i];
        }
        return res;
    }
    PlainText decrypt(const CipherText &ct) {
        Tensor<CipherText *> t(1, const_cast<CipherText *>(&ct));
        auto r = decrypt_tensor(t);
        PlainText out = *r[0];
        delete r[0];
        return out;
    }
    size_t decrypted_elements() const { return decrypted_; }

  private:
    CryptoSystem &cs_;
    SecretKey sk_;
    PublicKey pk_;
    size_t threshold_ = 0;
    Vector<SecretKeyShare> shares_;
    size_t decrypted_ = 0;
};

template <typename CryptoSystem, typename Client = LocalSMPCClient<CryptoSystem>>
class LocalCipherTextMultiplier {
  public:
    using CipherText = typename CryptoSystem::CipherText;
    using PlainText = typename CryptoSystem::PlainText;

    explicit LocalCipherTextMultiplier(Client &client) : client_m(client) {}
    // off (the default): the reference's sequence of calls; on: differences by subtraction, e*d added as a plaintext
    void set_direct_differences(bool on) { direct_differences_m = on; }
    bool direct_differences() const { return direct_differences_m; }
    // off (the default): the 2-D product expands into n m p element products as the reference does; on: one matrix triplet
    void set_matrix_triplets(bool on) { matrix_triplets_m = on; }
    bool matrix_triplets() const { return matrix_triplets_m; }

    CipherText multiply_ciphertexts(const CipherText &ct1, const CipherText &ct2) {
        Tensor<CipherText *> a(1, const_cast<CipherText *>(&ct1)), b(1, const_cast<CipherText *>(&ct2));
        auto r = handle_vector_ciphertext_mul(a, b);
        CipherText out = *r[0];
        delete r[0];
        return out;
    }

    // 0-D, 1-D (element-wise) and 2-D (matrix product) as in the reference (:40-112)
    Tensor<CipherText *> multiply_ciphertext_tensors(const Tensor<CipherText *> &ct1, const Tensor<CipherText *> &ct2) {
        if (ct1.is_zero_degree() && ct2.is_zero_degree())
            return Tensor<CipherText *>(new CipherText(multiply_ciphertexts(*ct1.get_value(), *ct2.get_value())));
        if (ct1.ndim() == 1) return handle_vector_ciphertext_mul(ct1, ct2);
        if (ct1.ndim() == 2) {
            // all n*m*p element products in one batch (:52-75), then one accumulation kernel
            // instead of the n*p*m serial nucomp loop (:85-101)
            const size_t n = ct1.shape()[0], m = ct1.shape()[1], p = ct2.shape()[1], nmp = n * m * p;
            if (ct2.shape()[0] != m) throw std::invalid_argument("Tensor shapes must be equal");
            if (matrix_triplets_m) return matrix_mul_triplet(ct1, ct2, n, m, p);
            Tensor<CipherText *> ct1_nmp(nmp, nullptr), ct2_nmp(nmp, nullptr);
            for (size_t i = 0; i < n; i++)
                for (size_t j = 0; j < m; j++)
                    for (size_t k = 0; k < p; k++) {
                        ct1_nmp[i * m * p + j * p + k] = ct1[i * m + j];
                        ct2_nmp[i * m * p + j * p + k] = ct2[j * p + k];
                    }
            auto res_nmp = handle_vector_ciphertext_mul(ct1_nmp, ct2_nmp);
            auto &cs = client_m.crypto_system();
            auto zero = cs.encrypt(client_m.network_public_key(), cs.make_plaintext(0));
            auto res = cs.accumulate_ciphertext_tensor(zero, res_nmp, n, m, p);
            for (size_t i = 0; i < nmp; i++) delete res_nmp[i];
            return res;
        }
        throw std::runtime_error("Not implemented");
    }

    // 2-D convolution of a ciphertext image x [B, H, W, C] with CIPHERTEXT filters w [kh, kw, C, Co], channels last, groups = 1:
    // one convolution triplet {[A], [Bf], [C] = [A * Bf]} and, convolution being bilinear, matrix_mul_triplet step for step:
    //   E = Dec(x - A), D = Dec(w - Bf);  [x * w] = (E * [Bf]) o ([A] * D) o [C] o f^(E * D)
    // which opens B H W C + kh kw C Co values, where the matrix triplet on the patch matrix opens n m + m p (every pixel kh kw
    // times, and the padding as encryptions of zero).  A batch B shares the one [Bf] and the one opened D: that is how many
    // images under the same private filters are meant to be run.  The reference has no convolution.
    Tensor<CipherText *> conv2d_ciphertext_tensors(const Tensor<CipherText *> &x, const Tensor<CipherText *> &w, const std::array<size_t, 2> &stride = {1, 1},
                                                   const std::array<size_t, 2> &pad = {0, 0}, const std::array<size_t, 2> &dilation = {1, 1}) {
        if (x.ndim() != 4 || w.ndim() != 4) throw std::invalid_argument("conv2d_ciphertext_tensors: both operands must be 4D");
        if (w.shape()[2] != x.shape()[3]) throw std::invalid_argument("conv2d_ciphertext_tensors: the channels of the filters and of the image differ");
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        auto triplet = client_m.get_beavers_conv2d_triplet(x.shape(), w.shape(), stride, pad, dilation);
        auto &a_tensor = triplet[0], &b_tensor = triplet[1], &c_tensor = triplet[2];
        auto x_sub_a = cs.sub_ciphertext_tensors(pk, x, a_tensor);
        auto w_sub_b = cs.sub_ciphertext_tensors(pk, w, b_tensor);
        auto e = client_m.decrypt_tensor(x_sub_a);
        auto d = client_m.decrypt_tensor(w_sub_b);
        auto e_b = cs.conv2d_ciphertext_filters_tensors(pk, e, b_tensor, stride, pad, dilation);
        auto a_d = cs.conv2d_plaintext_ciphertext_tensors(pk, d, a_tensor, stride, pad, dilation, 1);
        auto s1 = cs.add_ciphertext_tensors(pk, e_b, a_d);
        auto s2 = cs.add_ciphertext_tensors(pk, s1, c_tensor);
        auto e_d = cs.conv2d_plaintext_tensors(e, d, stride, pad, dilation);
        auto ct = cs.add_plaintext_tensor(pk, s2, e_d);
        for (size_t i = 0; i < x.num_elements(); i++) {
            delete a_tensor[i];
            delete x_sub_a[i];
            delete e[i];
        }
        for (size_t i = 0; i < w.num_elements(); i++) {
            delete b_tensor[i];
            delete w_sub_b[i];
            delete d[i];
        }
        for (size_t i = 0; i < ct.num_elements(); i++) {
            delete c_tensor[i];
            delete e_b[i];
            delete a_d[i];
            delete s1[i];
            delete s2[i];
            delete e_d[i];
        }
        return ct;
    }

    // p(x) element-wise for p = sum_j coef[j] X^j with plaintext coefficients (d + 1 of them, 1 <= d <= 8), over the integers
    // mod 2^k: with a power tuple ([a], .., [a^d]) per element, ONE opened value e = Dec(x - a) and one round whatever d, where
    // d - 1 chained products open 2 (d - 1) values in d - 1 rounds.  The reference has no such operation (ComputeOperation's
    // POLYNOMIAL_EVALUATION is commented out, include/node/compute_request_handler.hpp:74).  Fixed-point scales are the
    // caller's: coef[j] comes pre-scaled so that every term carries one scale.  0-D and 1-D tensors; higher ranks are
    // flattened and the result reshaped.
    Tensor<CipherText *> evaluate_polynomial_ciphertext_tensor(const Tensor<PlainText *> &coef, const Tensor<CipherText *> &x) {
        if (coef.num_elements() < 2) throw std::invalid_argument("evaluate_polynomial_ciphertext_tensor: a polynomial of degree 1 to 8");
        return open_and_close(x, client_m.get_beavers_power_tuples(x.num_elements(), coef.num_elements() - 1),
                              [&](const Tensor<PlainText *> &e, const Vector<Tensor<CipherText *>> &powers) {
                                  return client_m.crypto_system().poly_close_ciphertext_tensor(client_m.network_public_key(), coef, e, powers);
                              });
    }
    // x^2 element-wise: the polynomial (0, 0, 1), one opened value per element where the Beaver product x * x opens two
    Tensor<CipherText *> square_ciphertext_tensor(const Tensor<CipherText *> &x) {
        PlainText zero(0ul), one(1ul);
        Tensor<PlainText *> coef(3, &zero);
        coef[2] = &one;
        return evaluate_polynomial_ciphertext_tensor(coef, x);
    }

    // floor(x / D) element-wise for public divisors D, 1 <= D < 2^(k-1), x read as its centred residue: with a division pair
    // ([r], [r_q]) per element, ONE opened value e = Dec(x - r) and one round; the result is the floor quotient or one less
    // unless s(r) + s(e) wraps, which has probability |x| / 2^k per element (the caller keeps |x| <= 2^(k-1-sigma)).  div holds
    // one divisor, or one per channel of a channels-last tensor (its count divides x's), or one per element.  0-D and 1-D
    // tensors; higher ranks are flattened and the result reshaped.
    Tensor<CipherText *> divide_ciphertext_tensor_by_plaintext(const Tensor<CipherText *> &x, const Tensor<PlainText *> &div) {
        auto &cs = client_m.crypto_system();
        Tensor<PlainText *> d = div.is_zero_degree() ? Tensor<PlainText *>(1, div.get_value()) : div;
        d.flatten();
        cs.check_divisors(d, x.num_elements());
        return open_and_close(x, client_m.get_division_pairs(x.num_elements(), d),
                              [&](const Tensor<PlainText *> &e, const Vector<Tensor<CipherText *>> &pairs) {
                                  return cs.div_close_ciphertext_tensor(client_m.network_public_key(), e, d, pairs[1]);
                              });
    }
    // floor(x / 2^t): the rescale after a product of two fixed-point values, 1 <= t <= k - 2
    Tensor<CipherText *> truncate_ciphertext_tensor(const Tensor<CipherText *> &x, uint32_t t) {
        if (t == 0 || t + 2 > client_m.crypto_system().message_bits()) throw std::invalid_argument("truncate_ciphertext_tensor: 1 <= t <= k - 2");
        PlainText D;
        mpz_setbit(D.get(), t);
        return divide_ciphertext_tensor_by_plaintext(x, Tensor<PlainText *>(1, &D));
    }
    // average pooling, channels last: sum_pool2d_ciphertext_tensor over kernel[0] x kernel[1] windows, then the division by
    // kernel[0] kernel[1]: the floor of the mean or one less.  Padding counts as zeros in the mean.
    Tensor<CipherText *> avg_pool2d_ciphertext_tensor(const Tensor<CipherText *> &x, const std::array<size_t, 2> &kernel,
                                                      const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad = {0, 0}) {
        auto &cs = client_m.crypto_system();
        auto sums = cs.sum_pool2d_ciphertext_tensor(client_m.network_public_key(), x, kernel, stride, pad);
        PlainText D((unsigned long)(kernel[0] * kernel[1]));
        auto res = divide_ciphertext_tensor_by_plaintext(sums, Tensor<PlainText *>(1, &D));
        Tensor<CipherText *> flat = sums;
        flat.flatten();
        for (size_t i = 0; i < flat.num_elements(); i++) delete flat[i];
        return res;
    }

    // floor(x / D) EXACTLY, element-wise for small public divisors D, 1 <= D <= 4096 and D < 2^(k-1), x read as its centred
    // residue: with an exact-division tuple per element, ONE opened value e = Dec(x - r) and one round; the closing step copies
    // the entry s(e) mod D of the element's tuple and adds the plaintext floor(s(e) / D).  Wrong only where s(r) + s(e) wraps,
    // which has probability |x| / 2^k per element (the caller keeps |x| <= 2^(k-1-sigma)), as for the inexact division.  Nearest
    // adds the plaintext floor(D / 2) first: the nearest integer to x / D, ties up.  div holds one divisor, or one per channel
    // of a channels-last tensor (its count divides x's), or one per element; a tuple is max(D) ciphertexts per element.  0-D
    // and 1-D tensors; higher ranks are flattened and the result reshaped.
    enum class Rounding { Floor, Nearest };
    Tensor<CipherText *> divide_exact_ciphertext_tensor_by_plaintext(const Tensor<CipherText *> &x, const Tensor<PlainText *> &div,
                                                                     Rounding rounding = Rounding::Floor) {
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        Tensor<PlainText *> d = div.is_zero_degree() ? Tensor<PlainText *>(1, div.get_value()) : div;
        d.flatten();
        const size_t n = x.num_elements();
        (void)cs.check_small_divisors(d, n);
        auto close = [&](const Tensor<PlainText *> &e, const Vector<Tensor<CipherText *>> &tuples) {
            return cs.divx_close_ciphertext_tensor(pk, e, d, tuples[1]);
        };
        if (rounding == Rounding::Floor) return open_and_close(x, client_m.get_exact_division_tuples(n, d), close);
        // x + floor(D / 2) element-wise, then the floor
        std::vector<PlainText> halves(d.num_elements());
        for (size_t i = 0; i < d.num_elements(); i++) mpz_fdiv_q_2exp(halves[i].get(), d[i]->get(), 1);
        Tensor<PlainText *> addend(n, nullptr);
        for (size_t i = 0; i < n; i++) addend[i] = &halves[i % halves.size()];
        Tensor<CipherText *> flat = x.is_zero_degree() ? Tensor<CipherText *>(1, x.get_value()) : x;
        flat.flatten();
        auto shifted = cs.add_plaintext_tensor(pk, flat, addend);
        auto res = open_and_close(shifted, client_m.get_exact_division_tuples(n, d), close);
        for (size_t i = 0; i < n; i++) delete shifted[i];
        if (x.is_zero_degree()) return Tensor<CipherText *>(res.at(0));
        res.reshape(x.shape());
        return res;
    }
    // floor(x / 2^t) EXACTLY: the rescale after a product of two fixed-point values.  t <= 12 takes one round; a larger t takes
    // ceil(t / 12) rounds of near-equal shifts (t = 16: 8 + 8, 512 tuple entries per element, not 12 + 4 with 4112), which is
    // exact because nested floors by positive divisors compose: floor(floor(x / a) / b) = floor(x / (a b)).  1 <= t <= k - 2.
    Tensor<CipherText *> truncate_exact_ciphertext_tensor(const Tensor<CipherText *> &x, uint32_t t) {
        if (t == 0 || t + 2 > client_m.crypto_system().message_bits()) throw std::invalid_argument("truncate_exact_ciphertext_tensor: 1 <= t <= k - 2");
        const uint32_t rounds = (t + 11) / 12;
        Tensor<CipherText *> cur = x;
        for (uint32_t i = 0; i < rounds; i++) {
            const uint32_t shift = t / rounds + (i < t % rounds ? 1 : 0);
            PlainText D;
            mpz_setbit(D.get(), shift);
            auto next = divide_exact_ciphertext_tensor_by_plaintext(cur, Tensor<PlainText *>(1, &D));
            if (i > 0) free_elements(cur);
            cur = next;
        }
        return cur;
    }
    // x - D floor(x / D) element-wise, in [0, D): one exact division, then a scaling by D and a difference
    Tensor<CipherText *> remainder_ciphertext_tensor(const Tensor<CipherText *> &x, const Tensor<PlainText *> &div) {
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        Tensor<PlainText *> d = div.is_zero_degree() ? Tensor<PlainText *>(1, div.get_value()) : div;
        d.flatten();
        const size_t n = x.num_elements();
        auto y = divide_exact_ciphertext_tensor_by_plaintext(x, d);
        Tensor<CipherText *> flat = x.is_zero_degree() ? Tensor<CipherText *>(1, x.get_value()) : x, yf = y.is_zero_degree() ? Tensor<CipherText *>(1, y.get_value()) : y;
        flat.flatten();
        yf.flatten();
        Tensor<PlainText *> scale(n, nullptr);
        for (size_t i = 0; i < n; i++) scale[i] = d[i % d.num_elements()];
        auto dy = cs.scal_ciphertext_tensors(pk, scale, yf);
        auto res = cs.sub_ciphertext_tensors(pk, flat, dy);
        for (size_t i = 0; i < n; i++) {
            delete yf[i];
            delete dy[i];
        }
        if (x.is_zero_degree()) return Tensor<CipherText *>(res.at(0));
        res.reshape(x.shape());
        return res;
    }
    // x = sum_i digit_i 2^(digit_bits i): n_digits - 1 digits in [0, 2^digit_bits) and the signed top part, least significant
    // first, each of x's shape; 1 <= digit_bits <= 12, n_digits >= 2.  One exact division by 2^digit_bits per digit below the
    // top: the quotient is carried on and the digit is what the division leaves, cur - 2^digit_bits quotient.
    Vector<Tensor<CipherText *>> decompose_ciphertext_tensor(const Tensor<CipherText *> &x, uint32_t digit_bits, uint32_t n_digits) {
        if (digit_bits == 0 || digit_bits > 12 || n_digits < 2) throw std::invalid_argument("decompose_ciphertext_tensor: 1 <= digit_bits <= 12, n_digits >= 2");
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        const size_t n = x.num_elements();
        PlainText D;
        mpz_setbit(D.get(), digit_bits);
        Tensor<PlainText *> scale(n, &D);
        Tensor<CipherText *> cur = x.is_zero_degree() ? Tensor<CipherText *>(1, x.get_value()) : x;
        cur.flatten();
        Vector<Tensor<CipherText *>> out;
        for (uint32_t i = 0; i + 1 < n_digits; i++) {
            auto q = divide_exact_ciphertext_tensor_by_plaintext(cur, Tensor<PlainText *>(1, &D));
            auto dq = cs.scal_ciphertext_tensors(pk, scale, q);
            auto digit = cs.sub_ciphertext_tensors(pk, cur, dq);
            free_elements(dq);
            if (i > 0) free_elements(cur);
            if (!x.is_zero_degree()) digit.reshape(x.shape());
            out.push_back(digit);
            cur = q;
        }
        if (!x.is_zero_degree()) cur.reshape(x.shape());
        out.push_back(cur);
        return out;
    }
    // average pooling, channels last, EXACT: sum_pool2d_ciphertext_tensor over kernel[0] x kernel[1] windows, then the exact
    // division by kernel[0] kernel[1] (at most 4096): the floor of the mean.  Padding counts as zeros in the mean.
    Tensor<CipherText *> avg_pool2d_exact_ciphertext_tensor(const Tensor<CipherText *> &x, const std::array<size_t, 2> &kernel,
                                                            const std::array<size_t, 2> &stride, const std::array<size_t, 2> &pad = {0, 0}) {
        auto &cs = client_m.crypto_system();
        auto sums = cs.sum_pool2d_ciphertext_tensor(client_m.network_public_key(), x, kernel, stride, pad);
        PlainText D((unsigned long)(kernel[0] * kernel[1]));
        auto res = divide_exact_ciphertext_tensor_by_plaintext(sums, Tensor<PlainText *>(1, &D));
        free_elements(sums);
        return res;
    }

    // g[x mod 2^b] element-wise for a public table g of 2^b plaintexts ([2^b], or [n_tab, 2^b] with element i taking table i mod
    // n_tab), 1 <= b <= 12, b <= k: with a lookup tuple per element, ONE opened value e = Dec(x - r), one round, exact, no
    // failure probability; the closing step copies the entry e mod 2^b of the element's tuple.  x must lie in the b-bit range
    // for the result to be g[x]; a b-bit signed value is read as its two's-complement index.  A tuple is 2^b ciphertexts (1344
    // bytes each on the device) per element.  0-D and 1-D tensors; higher ranks are flattened and the result reshaped.
    Tensor<CipherText *> lookup_ciphertext_tensor(const Tensor<PlainText *> &table, const Tensor<CipherText *> &x) {
        return open_and_close(x, client_m.get_lookup_tuples(x.num_elements(), table),
                              [&](const Tensor<PlainText *> &e, const Vector<Tensor<CipherText *>> &tuples) {
                                  return client_m.crypto_system().lut_select_ciphertext_tensor(e, tuples[1]);
                              });
    }
    // A piecewise polynomial element-wise, over the (shift + bits)-bit window of x: `table` holds 2^bits pieces of d + 1
    // coefficients ([2^bits, d + 1], or [n_tab, 2^bits, d + 1] with element i taking table i mod n_tab; make_spline_table of
    // spline_table.hpp builds one from a function), piece p evaluating sum_i c[p][i] (x - o(p))^i mod 2^k from its origin
    // o(p) = sigma(p) 2^shift.  With a spline tuple per element, ONE opened value e = Dec(x - r) and one round; the tuple is
    // 2^bits (d + 1) ciphertexts per element, not 2^(shift + bits).  The result is the value of the element's own piece or of the
    // piece below (the carry of the low shift bits is lost; shift = 0: always its own), so every piece must approximate the
    // function on two segments, and x must stay out of the lowest segment.  0-D and 1-D tensors; higher ranks are flattened and
    // the result reshaped.
    Tensor<CipherText *> evaluate_spline_ciphertext_tensor(const Tensor<PlainText *> &table, const Tensor<CipherText *> &x, uint32_t bits,
                                                           uint32_t shift) {
        return open_and_close(x, client_m.get_spline_tuples(x.num_elements(), table, bits, shift),
                              [&](const Tensor<PlainText *> &e, const Vector<Tensor<CipherText *>> &tuples) {
                                  return client_m.crypto_system().spline_close_ciphertext_tensor(e, tuples[1], bits, shift);
                              });
    }
    // max(x, 0) for `bits`-bit signed values x, exactly: the table holds v for 0 < v < 2^(bits-1) and 0 otherwise
    Tensor<CipherText *> relu_ciphertext_tensor(const Tensor<CipherText *> &x, uint32_t bits) {
        if (bits == 0 || bits > COFHE_HIP_LUT_MAX_BITS) throw std::invalid_argument("relu_ciphertext_tensor: 1 <= bits <= 12");
        const size_t size = (size_t)1 << bits;
        std::vector<PlainText> vals(size);
        Tensor<PlainText *> table(size, nullptr);
        for (size_t v = 0; v < size; v++) {
            if (v < size / 2) mpz_set_ui(vals[v].get(), (unsigned long)v);
            table[v] = &vals[v];
        }
        return lookup_ciphertext_tensor(table, x);
    }
    // max(a, b) element-wise for `bits`-bit signed values: b + relu(a - b), the difference a (bits + 1)-bit signed value, so
    // 1 <= bits <= 11; one opened value per element
    Tensor<CipherText *> max_ciphertext_tensors(const Tensor<CipherText *> &a, const Tensor<CipherText *> &b, uint32_t bits) {
        if (bits == 0 || bits + 1 > COFHE_HIP_LUT_MAX_BITS) throw std::invalid_argument("max_ciphertext_tensors: 1 <= bits <= 11");
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        auto diff = cs.sub_ciphertext_tensors(pk, a, b);
        auto pos = relu_ciphertext_tensor(diff, bits + 1);
        auto res = cs.add_ciphertext_tensors(pk, b, pos);
        if (diff.is_zero_degree()) {
            delete diff.get_value();
            delete pos.get_value();
        } else {
            for (size_t i = 0; i < diff.num_elements(); i++) {
                delete diff[i];
                delete pos[i];
            }
        }
        return res;
    }
    // max pooling of `bits`-bit signed values, channels last ([B, H, W, C] -> [B, Ho, Wo, C]): a pairwise tournament
    // over the kernel[0] kernel[1] taps of a window, ceil(log2(taps)) rounds of ONE batched max_ciphertext_tensors call each (an
    // odd tap passes through), taps - 1 lookups and opened values per output.  Without padding the taps are gathered by pointer
    // arithmetic on the host tensor and nothing is copied until the cryptosystem's upload gathers them on the device.  With
    // pad != {0, 0} (each smaller than its kernel extent) the taps are window_taps_ciphertext_tensor of x with a fill of ONE fresh
    // Enc(-2^(bits - 1)), the least `bits`-bit value: padding never wins, and a window wholly in the padding returns that value.
    // The padding elements are copies of one ciphertext (they share its randomness); every output is the result of a lookup
    // and carries randomness of its own.
    Tensor<CipherText *> max_pool2d_ciphertext_tensor(const Tensor<CipherText *> &x, const std::array<size_t, 2> &kernel,
                                                      const std::array<size_t, 2> &stride, uint32_t bits, const std::array<size_t, 2> &pad = {0, 0}) {
        if (x.is_zero_degree() || x.ndim() != 4) throw std::invalid_argument("max_pool2d_ciphertext_tensor: a [B, H, W, C] tensor");
        const size_t B = x.shape()[0], H = x.shape()[1], W = x.shape()[2], C = x.shape()[3], kh = kernel[0], kw = kernel[1];
        const bool padded = pad[0] != 0 || pad[1] != 0;
        if (kh == 0 || kw == 0 || stride[0] == 0 || stride[1] == 0 || kh > H + 2 * pad[0] || kw > W + 2 * pad[1])
            throw std::invalid_argument("max_pool2d_ciphertext_tensor: the window lies inside the image, the strides are not 0");
        if (padded && (bits == 0 || bits + 1 > COFHE_HIP_LUT_MAX_BITS)) throw std::invalid_argument("max_ciphertext_tensors: 1 <= bits <= 11");
        const size_t Ho = (H + 2 * pad[0] - kh) / stride[0] + 1, Wo = (W + 2 * pad[1] - kw) / stride[1] + 1, n_out = B * Ho * Wo * C;
        struct Tap {
            Tensor<CipherText *> t;
            bool owned;                              // a result of an earlier round or a copy, not elements of x
        };
        std::vector<Tap> taps;
        if (padded) {
            auto &cs = client_m.crypto_system();
            const CipherText least = cs.encrypt(client_m.network_public_key(), cs.make_plaintext(-(float)((size_t)1 << (bits - 1))));
            Tensor<CipherText *> all = cs.window_taps_ciphertext_tensor(x, kernel, stride, pad, {1, 1}, &least);      // [kh, kw, B, Ho, Wo, C]
            for (size_t tap = 0; tap < kh * kw; tap++) {
                Tensor<CipherText *> t(n_out, nullptr);
                for (size_t i = 0; i < n_out; i++) t[i] = all[tap * n_out + i];
                taps.push_back(Tap{t, true});
            }
        }
        for (size_t dy = 0; dy < (padded ? 0 : kh); dy++)
            for (size_t dx = 0; dx < kw; dx++) {
                Tensor<CipherText *> t(n_out, nullptr);
                size_t o = 0;
                for (size_t b = 0; b < B; b++)
                    for (size_t oy = 0; oy < Ho; oy++)
                        for (size_t ox = 0; ox < Wo; ox++)
                            for (size_t c = 0; c < C; c++) t[o++] = x[((b * H + oy * stride[0] + dy) * W + ox * stride[1] + dx) * C + c];
                taps.push_back(Tap{t, false});
            }
        while (taps.size() > 1) {
            const size_t pairs = taps.size() / 2;
            Tensor<CipherText *> lhs(pairs * n_out, nullptr), rhs(pairs * n_out, nullptr);
            for (size_t p = 0; p < pairs; p++)
                for (size_t i = 0; i < n_out; i++) {
                    lhs[p * n_out + i] = taps[2 * p].t[i];
                    rhs[p * n_out + i] = taps[2 * p + 1].t[i];
                }
            auto m = max_ciphertext_tensors(lhs, rhs, bits);
            std::vector<Tap> next;
            for (size_t p = 0; p < pairs; p++) {
                Tensor<CipherText *> t(n_out, nullptr);
                for (size_t i = 0; i < n_out; i++) t[i] = m[p * n_out + i];
                next.push_back(Tap{t, true});
            }
            for (size_t p = 0; p < 2 * pairs; p++)
                if (taps[p].owned)
                    for (size_t i = 0; i < n_out; i++) delete taps[p].t[i];
            if (taps.size() % 2) next.push_back(taps.back());
            taps = std::move(next);
        }
        Tensor<CipherText *> res = taps[0].t;
        if (!taps[0].owned)                          // a 1 x 1 window: the caller owns copies, as of every result tensor
            for (size_t i = 0; i < n_out; i++) res[i] = new CipherText(*res[i]);
        res.reshape({B, Ho, Wo, C});
        return res;
    }

    // [x >= 0] element-wise (an encryption of 1 or 0) for x in the signed window of `bits` bits, 2 <= bits <= min(k, 64), exactly
    // and with no failure probability: with a comparison tuple per element, round 1 opens e = Dec(x - r) and composes, for the two
    // thresholds of e, the entries that their digits select; round 2 is ONE lookup of n + 1 bits over the 2 E products.  Three
    // opened values per element, and n 2^d + 2^(n + 2) ciphertexts of tuples for n = ceil(bits / d) digits where a lookup takes
    // 2^bits.  digit_bits = 0 picks the d that needs the fewest.  0-D and 1-D tensors; higher ranks are flattened and the result
    // reshaped.
    Tensor<CipherText *> is_nonnegative_ciphertext_tensor(const Tensor<CipherText *> &x, uint32_t bits, uint32_t digit_bits = 0) {
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        const uint32_t d = digit_bits ? digit_bits : cs.cmp_pick_digit_bits(bits);
        const uint32_t n = cs.cmp_shape(bits, d).digits;         // refuses d = 0 (no digit width fits) with everything else
        return open_and_close(x, client_m.get_comparison_tuples(x.num_elements(), bits, d),
                              [&](const Tensor<PlainText *> &e, const Vector<Tensor<CipherText *>> &tuples) {
                                  const size_t E = e.num_elements();
                                  auto closed = cs.cmp_close_ciphertext_tensor(e, tuples[1], bits, d);
                                  // g[v] = 1 for v < 2^n, the non-negative half of the (n + 1)-bit two's-complement range
                                  const size_t size = (size_t)2 << n;
                                  std::vector<PlainText> vals(size);
                                  Tensor<PlainText *> table(size, nullptr);
                                  for (size_t v = 0; v < size; v++) {
                                      if (v < size / 2) mpz_set_ui(vals[v].get(), 1ul);
                                      table[v] = &vals[v];
                                  }
                                  Tensor<CipherText *> s = closed.pairs;
                                  s.flatten();
                                  auto g = lookup_ciphertext_tensor(table, s);
                                  Tensor<CipherText *> ga(E, nullptr), gb(E, nullptr);
                                  Tensor<PlainText *> c(E, nullptr);
                                  for (size_t i = 0; i < E; i++) {
                                      ga[i] = g[2 * i];
                                      gb[i] = g[2 * i + 1];
                                      c[i] = new PlainText(mpz_sgn(closed.wrap[i]->get()) != 0 ? 0ul : 1ul);
                                  }
                                  // [x >= 0] = (1 - wrap) - g(S_A) + g(S_B)
                                  auto diff = cs.sub_ciphertext_tensors(pk, gb, ga);
                                  auto res = cs.add_plaintext_tensor(pk, diff, c);
                                  for (size_t i = 0; i < E; i++) {
                                      delete s[2 * i];
                                      delete s[2 * i + 1];
                                      delete closed.wrap[i];
                                      delete ga[i];
                                      delete gb[i];
                                      delete c[i];
                                      delete diff[i];
                                  }
                                  return res;
                              });
    }
    // max(x, 0) for x in the signed window of `bits` bits, 2 <= bits <= min(k, 64), exactly: x [x >= 0], the sign above and one
    // Beaver product; five opened values per element.  Shapes as above.
    Tensor<CipherText *> relu_wide_ciphertext_tensor(const Tensor<CipherText *> &x, uint32_t bits, uint32_t digit_bits = 0) {
        Tensor<CipherText *> flat = x.is_zero_degree() ? Tensor<CipherText *>(1, x.get_value()) : x;
        flat.flatten();
        auto nonneg = is_nonnegative_ciphertext_tensor(flat, bits, digit_bits);
        auto res = handle_vector_ciphertext_mul(flat, nonneg);
        for (size_t i = 0; i < nonneg.num_elements(); i++) delete nonneg[i];
        if (x.is_zero_degree()) return Tensor<CipherText *>(res.at(0));
        res.reshape(x.shape());
        return res;
    }
    // max(a, b) element-wise for values in the signed window of `bits` bits: b + relu(a - b), the difference a (bits + 1)-bit
    // signed value, so 1 <= bits <= 63 and bits + 1 <= k
    Tensor<CipherText *> max_wide_ciphertext_tensors(const Tensor<CipherText *> &a, const Tensor<CipherText *> &b, uint32_t bits, uint32_t digit_bits = 0) {
        if (bits == 0 || bits > 63) throw std::invalid_argument("max_wide_ciphertext_tensors: 1 <= bits <= 63");
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        auto diff = cs.sub_ciphertext_tensors(pk, a, b);
        auto pos = relu_wide_ciphertext_tensor(diff, bits + 1, digit_bits);
        auto res = cs.add_ciphertext_tensors(pk, b, pos);
        if (diff.is_zero_degree()) {
            delete diff.get_value();
            delete pos.get_value();
        } else {
            Tensor<CipherText *> fd = diff, fp = pos;
            fd.flatten();
            fp.flatten();
            for (size_t i = 0; i < fd.num_elements(); i++) {
                delete fd[i];
                delete fp[i];
            }
        }
        return res;
    }

    // element-wise products of two 1-D ciphertext tensors (:115-160), same order of calls
    Tensor<CipherText *> handle_vector_ciphertext_mul(const Tensor<CipherText *> &ct1, const Tensor<CipherText *> &ct2) {
        const size_t n = ct1.shape()[0];
        if (ct2.num_elements() != n) throw std::invalid_argument("Tensor shapes must be equal");
        if (direct_differences_m) return vector_mul_direct(ct1, ct2, n);
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        auto triplets = client_m.get_beavers_triplets(n);
        Tensor<CipherText *> a_tensor(n, nullptr), b_tensor(n, nullptr), c_tensor(n, nullptr);
        for (size_t i = 0; i < n; i++) {
            a_tensor[i] = triplets.at(i, 0);
            b_tensor[i] = triplets.at(i, 1);
            c_tensor[i] = triplets.at(i, 2);
        }
        auto neg_a_tensor = cs.negate_ciphertext_tensor(pk, a_tensor);
        auto neg_b_tensor = cs.negate_ciphertext_tensor(pk, b_tensor);
        auto ct1_neg_a = cs.add_ciphertext_tensors(pk, ct1, neg_a_tensor);
        auto ct2_neg_b = cs.add_ciphertext_tensors(pk, ct2, neg_b_tensor);
        auto pt1 = client_m.decrypt_tensor(ct1_neg_a);
        auto pt2 = client_m.decrypt_tensor(ct2_neg_b);
        auto pt1_pt2 = cs.multiply_plaintext_tensors(pt1, pt2);
        auto enc_pt1_pt2 = cs.encrypt_tensor(pk, pt1_pt2);
        auto pt1_b = cs.scal_ciphertext_tensors(pk, pt1, b_tensor);
        auto pt2_a = cs.scal_ciphertext_tensors(pk, pt2, a_tensor);
        auto s1 = cs.add_ciphertext_tensors(pk, pt1_b, pt2_a);
        auto s2 = cs.add_ciphertext_tensors(pk, s1, c_tensor);
        auto ct = cs.add_ciphertext_tensors(pk, s2, enc_pt1_pt2);
        for (size_t i = 0; i < n; i++) {
            delete triplets.at(i, 0);
            delete triplets.at(i, 1);
            delete triplets.at(i, 2);
            delete neg_a_tensor[i];
            delete neg_b_tensor[i];
            delete ct1_neg_a[i];
            delete ct2_neg_b[i];
            delete pt1[i];
            delete pt2[i];
            delete pt1_pt2[i];
            delete enc_pt1_pt2[i];
            delete pt1_b[i];
            delete pt2_a[i];
            delete s1[i];          // the reference leaks these two intermediates (:151-153)
            delete s2[i];
        }
        return ct;
    }

  private:
    // the elements of a tensor this class made, whatever its shape
    static void free_elements(const Tensor<CipherText *> &t) {
        Tensor<CipherText *> flat = t;
        flat.flatten();
        for (size_t i = 0; i < flat.num_elements(); i++) delete flat[i];
    }
    // The protocol of one opened value, behind the polynomial, the division and the lookup: e = Dec(x - material[0]) element-wise,
    // then close(e, material) makes the result, which takes x's shape.  material is what the client handed out for x's elements,
    // the mask first; it is used once, so every element of it is freed here, with the difference and the opened values.  A 0-D x
    // is one element and comes back 0-D; higher ranks are flattened and the result reshaped.
    template <typename Close>
    Tensor<CipherText *> open_and_close(const Tensor<CipherText *> &x, Vector<Tensor<CipherText *>> material, Close close) {
        auto &cs = client_m.crypto_system();
        Tensor<CipherText *> flat = x.is_zero_degree() ? Tensor<CipherText *>(1, x.get_value()) : x;
        flat.flatten();
        auto x_sub_m = cs.sub_ciphertext_tensors(client_m.network_public_key(), flat, material[0]);
        auto e = client_m.decrypt_tensor(x_sub_m);
        Tensor<CipherText *> ct = close(e, material);
        for (auto &t : material)
            for (size_t i = 0; i < t.num_elements(); i++) delete t[i];
        for (size_t i = 0; i < e.num_elements(); i++) {
            delete x_sub_m[i];
            delete e[i];
        }
        if (x.is_zero_degree()) return Tensor<CipherText *>(ct.at(0));
        ct.reshape(x.shape());
        return ct;
    }

    // the same product with x - a, y - b by subtraction and e*d as a plaintext addend: per element 2 compositions for the
    // differences (plus the folded c1) and one comb tree for f^(ed), against 2 (k + 1) + 2 compositions and an encryption
    Tensor<CipherText *> vector_mul_direct(const Tensor<CipherText *> &ct1, const Tensor<CipherText *> &ct2, size_t n) {
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        auto triplets = client_m.get_beavers_triplets(n);
        Tensor<CipherText *> a_tensor(n, nullptr), b_tensor(n, nullptr), c_tensor(n, nullptr);
        for (size_t i = 0; i < n; i++) {
            a_tensor[i] = triplets.at(i, 0);
            b_tensor[i] = triplets.at(i, 1);
            c_tensor[i] = triplets.at(i, 2);
        }
        auto ct1_sub_a = cs.sub_ciphertext_tensors(pk, ct1, a_tensor);
        auto ct2_sub_b = cs.sub_ciphertext_tensors(pk, ct2, b_tensor);
        auto pt1 = client_m.decrypt_tensor(ct1_sub_a);
        auto pt2 = client_m.decrypt_tensor(ct2_sub_b);
        auto pt1_pt2 = cs.multiply_plaintext_tensors(pt1, pt2);
        auto pt1_b = cs.scal_ciphertext_tensors(pk, pt1, b_tensor);
        auto pt2_a = cs.scal_ciphertext_tensors(pk, pt2, a_tensor);
        auto s1 = cs.add_ciphertext_tensors(pk, pt1_b, pt2_a);
        auto s2 = cs.add_ciphertext_tensors(pk, s1, c_tensor);
        auto ct = cs.add_plaintext_tensor(pk, s2, pt1_pt2);
        for (size_t i = 0; i < n; i++) {
            delete triplets.at(i, 0);
            delete triplets.at(i, 1);
            delete triplets.at(i, 2);
            delete ct1_sub_a[i];
            delete ct2_sub_b[i];
            delete pt1[i];
            delete pt2[i];
            delete pt1_pt2[i];
            delete pt1_b[i];
            delete pt2_a[i];
            delete s1[i];
            delete s2[i];
        }
        return ct;
    }

    // X (n x m) . Y (m x p) with one matrix triplet: n m + m p opened values instead of 2 n m p
    Tensor<CipherText *> matrix_mul_triplet(const Tensor<CipherText *> &x, const Tensor<CipherText *> &y, size_t n, size_t m, size_t p) {
        auto &cs = client_m.crypto_system();
        const auto &pk = client_m.network_public_key();
        auto triplet = client_m.get_beavers_matrix_triplet(n, m, p);
        auto &a_tensor = triplet[0], &b_tensor = triplet[1], &c_tensor = triplet[2];
        auto x_sub_a = cs.sub_ciphertext_tensors(pk, x, a_tensor);
        auto y_sub_b = cs.sub_ciphertext_tensors(pk, y, b_tensor);
        auto e = client_m.decrypt_tensor(x_sub_a);
        auto d = client_m.decrypt_tensor(y_sub_b);
        auto e_b = cs.matmul_plaintext_ciphertext_tensors(pk, e, b_tensor);
        auto a_d = cs.scal_ciphertext_tensors(pk, d, a_tensor);
        auto s1 = cs.add_ciphertext_tensors(pk, e_b, a_d);
        auto s2 = cs.add_ciphertext_tensors(pk, s1, c_tensor);
        auto e_d = cs.matmul_plaintext_tensors(e, d);
        auto ct = cs.add_plaintext_tensor(pk, s2, e_d);
        for (size_t i = 0; i < n * m; i++) {
            delete a_tensor[i];
            delete x_sub_a[i];
            delete e[i];
        }
        for (size_t i = 0; i < m * p; i++) {
            delete b_tensor[i];
            delete y_sub_b[i];
            delete d[i];
        }
        for (size_t i = 0; i < n * p; i++) {
            delete c_tensor[i];
            delete e_b[i];
            delete a_d[i];
            delete s1[i];
            delete s2[i];
            delete e_d[i];
        }
        return ct;
    }

    Client &client_m;
    bool direct_differences_m = false;
    bool matrix_triplets_m = false;
};

}  // namespace CoFHE
