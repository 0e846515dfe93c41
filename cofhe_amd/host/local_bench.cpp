// local_bench.cpp -- counterpart of the reference's local harness (benchmarks/local.cpp:65-215,
// benchmarks/benchmark.hpp) on the MI355X engine: same construction of inputs
// (make_plaintext(i+1), encrypt_tensor), same 1+49 chained operations with the per-iteration
// frees, first/last/average/median/total milliseconds per tag.  Additionally reports
// ciphertext-ops/s, the same chain with tensors kept resident in HBM, and writes the serialised
// bytes of the final tensor so a parity checker can compare them.
//
//   ./local_bench encrypt_decrypt [n m]          (reference default 64 64)
//   ./local_bench ciphertext_matadd [n m]        (reference default 64 64)
//   ./local_bench scal_matmul [n m p [chain]]    (reference default 8 64 64, 50 chained products)
//   ./local_bench threshold [n m t parties]      (threshold decryption, default 16 16 2 3)
//   ./local_bench ciphertext_matmul [n m p [t parties]]   (Beaver-triplet ct x ct product, default 4 4 4)
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <ctime>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <set>
#include <string>
#include <thread>
#include <utility>

#include "hip_cryptosystem.hpp"
#include "smpc_local.hpp"

using namespace CoFHE;
using Clock = std::chrono::steady_clock;

// Same bookkeeping as the reference's Benchmark (benchmarks/benchmark.hpp:5-146): start / end stamp of every run, the
// printed summary, and save() -- the results file ./benchmark_results_<tag><date>.txt with the summary block and one
// "Start: .. End: .." line per run (benchmark.hpp:96-116).  The harness calls save() when LOCAL_BENCH_SAVE is set.
struct Benchmark {
    using TP = std::chrono::time_point<std::chrono::high_resolution_clock>;
    std::string tag;
    std::vector<std::pair<TP, TP>> timestamps;
    std::vector<double> ms;
    explicit Benchmark(std::string t) : tag(std::move(t)) {}
    template <typename F>
    void run(F &&f, int times) {
        for (int i = 0; i < times; i++) {
            const TP t0 = std::chrono::high_resolution_clock::now();
            f();
            const TP t1 = std::chrono::high_resolution_clock::now();
            timestamps.emplace_back(t0, t1);
            ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
    }
    double total() const { return std::accumulate(ms.begin(), ms.end(), 0.0); }
    double median() const {
        std::vector<double> s = ms;
        std::sort(s.begin(), s.end());
        return s[s.size() / 2];
    }
    void summary(std::ostream &o) const {
        o << "======================" << std::endl;
        o << "Benchmark summary " + tag << std::endl;
        o << "Number of runs: " << ms.size() << std::endl;
        o << "First run time: " << ms.front() << "ms" << std::endl;
        o << "Last run time: " << ms.back() << "ms" << std::endl;
        o << "Average time: " << total() / ms.size() << "ms" << std::endl;
        o << "Median time: " << median() << "ms" << std::endl;
        o << "Total time: " << total() << "ms" << std::endl;
        o << "======================" << std::endl;
    }
    void print_summary() const {
        if (ms.empty()) return;
        std::cout << "Benchmark: " << tag << "\n  runs " << ms.size() << " first " << ms.front() << " ms, last " << ms.back()
                  << " ms, average " << total() / ms.size() << " ms, median " << median() << " ms, total " << total()
                  << " ms" << std::endl;
        if (getenv("LOCAL_BENCH_SAVE")) save();
    }
    std::string save() const {
        if (ms.empty()) return "";
        time_t now = time(nullptr);
        struct tm tstruct = *localtime(&now);
        char buf[80];
        strftime(buf, sizeof(buf), "%Y-%m-%d.%X", &tstruct);
        std::string name = tag;
        for (char &ch : name)
            if (ch == ' ' || ch == '/' || ch == ':' || ch == '(' || ch == ')' || ch == '<' || ch == '>' || ch == '*') ch = '_';
        const std::string filename = "./benchmark_results_" + name + buf + ".txt";
        std::ofstream file(filename, std::ios::app);
        summary(file);
        for (const auto &se : timestamps)
            file << "Start: " << se.first.time_since_epoch().count() << " End: " << se.second.time_since_epoch().count() << std::endl;
        return filename;
    }
};

template <typename T>
static void free_all(Tensor<T *> t) {
    t.flatten();
    for (size_t i = 0; i < t.num_elements(); i++) delete t.at(i);
}

static void bench_matadd(size_t n, size_t m) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    Tensor<CS::PlainText *> pt1(n, m, nullptr), pt2(n, m, nullptr);
    pt1.flatten(); pt2.flatten();
    for (size_t i = 0; i < n * m; i++) {
        pt1.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
        pt2.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
    }
    pt1.reshape({n, m}); pt2.reshape({n, m});
    auto ct1 = cs.encrypt_tensor(pk, pt1);
    auto ct2 = cs.encrypt_tensor(pk, pt2);
    Benchmark b("ciphertext_matadd (API: Tensor<CipherText*> in and out each op)");
    std::string final_bytes;
    double api_chain_ms = 0, api_ser_ms = 0;
    b.run([&]() {
        auto t0 = Clock::now();
        auto res = cs.add_ciphertext_tensors(pk, ct1, ct2);
        for (int i = 0; i < 49; ++i) {
            auto res_c = cs.add_ciphertext_tensors(pk, res, ct2);
            free_all(res);
            res = res_c;
        }
        cs.synchronize();
        auto t1 = Clock::now();
        final_bytes = cs.serialize_ciphertext_tensor(res);
        free_all(res);
        api_chain_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        api_ser_ms = std::chrono::duration<double, std::milli>(Clock::now() - t1).count();
    }, 1);
    std::cout << "  of which 50 API calls " << api_chain_ms << " ms, serialising the result " << api_ser_ms << " ms" << std::endl;
    b.print_summary();
    std::cout << "  " << 50.0 * n * m / (b.ms[0] * 1e-3) << " ciphertext-ops/s (host marshalling included)" << std::endl;
    Benchmark r("ciphertext_matadd (tensors resident in HBM)");
    std::string resident_bytes;
    r.run([&]() {
        auto d1 = cs.upload(ct1);
        auto d2 = cs.upload(ct2);
        auto t0 = Clock::now();
        auto res = cs.add_ciphertext_tensors(d1, d2);
        for (int i = 0; i < 49; ++i) res = cs.add_ciphertext_tensors(res, d2);
        cs.synchronize();
        double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        std::cout << "  resident chain of 50: " << ms << " ms, " << 50.0 * n * m / (ms * 1e-3) << " ciphertext-ops/s" << std::endl;
        auto back = cs.download(res);
        resident_bytes = cs.serialize_ciphertext_tensor(back);
        free_all(back);
    }, 1);
    r.print_summary();
    std::cout << "  API chain and resident chain agree: " << (final_bytes == resident_bytes ? "yes" : "NO") << std::endl;
    std::ofstream("local_bench_matadd_ct1.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(ct1);
    std::ofstream("local_bench_matadd_ct2.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(ct2);
    std::ofstream("local_bench_matadd_out.bin", std::ios::binary) << final_bytes;
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    free_all(pt1); free_all(pt2); free_all(ct1); free_all(ct2);
    std::cout << "n: " << n << " m: " << m << std::endl;
}

static void bench_scal_matmul(size_t n, size_t m, size_t p, int chain) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    Tensor<CS::PlainText *> pt1(n, m, nullptr), pt2(m, p, nullptr);
    pt1.flatten(); pt2.flatten();
    for (size_t i = 0; i < n * m; i++) pt1.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
    for (size_t i = 0; i < m * p; i++) pt2.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
    pt1.reshape({n, m}); pt2.reshape({m, p});
    auto ct1 = cs.encrypt_tensor(pk, pt1);
    // the reference draws a fresh Enc(0) inside every product (tensor_ops.inl:352); a fixed one makes the run
    // reproducible for the parity checker
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    if (m != p) chain = 1;                                   // the chain re-feeds the n x p result as the n x m operand
    Benchmark b("scal_matmul (1 + " + std::to_string(chain - 1) + " chained products, benchmarks/local.cpp:177-197)");
    std::string final_bytes;
    b.run([&]() {
        auto res = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
        for (int i = 0; i < chain - 1; ++i) {
            auto res_c = cs.scal_ciphertext_tensors(pk, pt2, res, &zero);
            free_all(res);
            res = res_c;
        }
        final_bytes = cs.serialize_ciphertext_tensor(res);
        free_all(res);
    }, 1);
    b.print_summary();
    std::cout << "  " << (double)chain * n * p / (b.ms[0] * 1e-3) << " output ciphertexts/s" << std::endl;
    std::ofstream("local_bench_scal_s.bin", std::ios::binary) << cs.serialize_plaintext_tensor(pt2);
    std::ofstream("local_bench_scal_cts.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(ct1);
    {
        Tensor<CS::CipherText *> zt(1, &zero);
        std::ofstream("local_bench_scal_zero.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(zt);
    }
    std::ofstream("local_bench_scal_out.bin", std::ios::binary) << final_bytes;
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    free_all(pt1); free_all(pt2); free_all(ct1);
    std::cout << "n: " << n << " m: " << m << " p: " << p << " chain: " << chain << std::endl;
}

// counterpart of benchmark_encrypt_decrypt (benchmarks/local.cpp:22-63), with the check the
// reference omits: every plaintext must come back
static void bench_encrypt_decrypt(size_t n, size_t m) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    Tensor<CS::PlainText *> pts(n, m, nullptr);
    pts.flatten();
    for (size_t i = 0; i < n * m; i++) pts.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
    pts.reshape({n, m});
    Benchmark b("encrypt_decrypt");
    bool ok = true;
    double enc_first_ms = 0, enc_again_ms = 0, dec_ms = 0;
    b.run([&]() {
        // whole encrypt_tensor calls, h^r and pk^r included: the first builds the fixed-base tables of h and pk
        // (one chain of ~1000 squarings each), later calls find them in the context
        auto t0 = Clock::now();
        auto ct0 = cs.encrypt_tensor(pk, pts);
        cs.synchronize();
        auto t1 = Clock::now();
        auto ct = cs.encrypt_tensor(pk, pts);
        cs.synchronize();
        auto t2 = Clock::now();
        free_all(ct0);
        auto res = cs.decrypt_tensor(sk, ct);
        auto t3 = Clock::now();
        enc_first_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        enc_again_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
        dec_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
        ct.flatten(); res.flatten();
        for (size_t i = 0; i < ct.num_elements(); i++) {
            if (cs.get_float_from_plaintext(*res.at(i)) != (float)(i + 1)) ok = false;
            delete res.at(i);
            delete ct.at(i);
        }
    }, 1);
    // homomorphic identities through the whole stack: Dec(Enc a + Enc b) = a + b, Dec(3 * Enc a) = 3a
    {
        auto a = cs.encrypt(pk, cs.make_plaintext(230)), bb = cs.encrypt(pk, cs.make_plaintext(20));
        auto sum = cs.add_ciphertexts(pk, a, bb);
        auto tri = cs.scal_ciphertext(pk, cs.make_plaintext(3), a);
        auto neg = cs.scal_ciphertext(pk, cs.make_plaintext(-1), a);
        if (cs.get_float_from_plaintext(cs.decrypt(sk, sum)) != 250.0f) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, tri)) != 690.0f) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, neg)) != -230.0f) ok = false;
    }
    // the 0-D tensor branches (tensor_ops.inl:199-202, 275-278) call the scalar forms: randomised like the reference's ...
    {
        auto a = cs.encrypt(pk, cs.make_plaintext(7)), bb = cs.encrypt(pk, cs.make_plaintext(5));
        auto three = cs.make_plaintext(3);
        Tensor<CS::CipherText *> ta(&a), tb(&bb);
        Tensor<CS::PlainText *> ts(&three);
        auto sum = cs.add_ciphertext_tensors(pk, ta, tb);
        auto tri = cs.scal_ciphertext_tensors(pk, ts, ta);
        if (!sum.is_zero_degree() || !tri.is_zero_degree()) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *sum.get_value())) != 12.0f) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *tri.get_value())) != 21.0f) ok = false;
        // a second call gives a different ciphertext of the same value (fresh r)
        auto sum2 = cs.add_ciphertext_tensors(pk, ta, tb);
        if (sum2.get_value()->c1() == sum.get_value()->c1()) ok = false;
        delete sum.get_value(); delete sum2.get_value(); delete tri.get_value();
        // ... and deterministic when asked, so that a checker can compare bytes
        cs.set_rerandomize(false);
        auto dsum = cs.add_ciphertext_tensors(pk, ta, tb);
        auto dtri = cs.scal_ciphertext_tensors(pk, ts, ta);
        auto one = [&](const CS::CipherText &c) { CS::CipherText cc = c; Tensor<CS::CipherText *> t(1, &cc); return cs.serialize_ciphertext_tensor(t); };
        std::ofstream("local_bench_scalar_a.bin", std::ios::binary) << one(a);
        std::ofstream("local_bench_scalar_b.bin", std::ios::binary) << one(bb);
        std::ofstream("local_bench_scalar_sum.bin", std::ios::binary) << one(*dsum.get_value());
        std::ofstream("local_bench_scalar_tri.bin", std::ios::binary) << one(*dtri.get_value());
        delete dsum.get_value(); delete dtri.get_value();
        cs.set_rerandomize(true);
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    b.print_summary();
    free_all(pts);
    std::cout << "  encrypt_tensor (h^r, pk^r included): first call " << enc_first_ms << " ms (builds the tables of h and pk), next call "
              << enc_again_ms << " ms = " << n * m / (enc_again_ms * 1e-3) << " ciphertexts/s; decrypt_tensor " << dec_ms << " ms" << std::endl;
    std::cout << "  roundtrip and homomorphic checks: " << (ok ? "ok" : "FAILED") << std::endl;
    std::cout << "n: " << n << " m: " << m << std::endl;
    if (!ok) throw std::runtime_error("decryption mismatch");
}

// fresh randomness per element (TensorRandomness::PerElement): encrypt_tensor gives every ciphertext its own r, the tensor
// operations re-randomise their outputs, rerandomize_ciphertext_tensor does it on request; everything decrypts as before
static void bench_fresh_randomness(size_t n) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    Tensor<CS::PlainText *> pts(n, nullptr);
    std::vector<float> want(n);
    for (size_t i = 0; i < n; i++) {
        want[i] = (float)((long)i - (long)(n / 2));
        pts.at(i) = new CS::PlainText(cs.make_plaintext(want[i]));
    }
    bool ok = true;
    auto c1_text = [](const CS::CipherText &c) { return c.c1().a().str() + " " + c.c1().b().str(); };
    auto distinct_c1 = [&](const Tensor<CS::CipherText *> &t) {
        std::set<std::string> seen;
        for (size_t i = 0; i < t.num_elements(); i++) seen.insert(c1_text(*t[i]));
        return seen.size() == t.num_elements();
    };
    auto decrypts_to = [&](const Tensor<CS::CipherText *> &t, float factor) {
        auto res = cs.decrypt_tensor(sk, t);
        bool good = true;
        for (size_t i = 0; i < n; i++) {
            if (cs.get_float_from_plaintext(*res.at(i)) != factor * want[i]) good = false;
            delete res.at(i);
        }
        return good;
    };
    auto shared = cs.encrypt_tensor(pk, pts);                 // default mode: one r for the tensor
    cs.synchronize();
    for (size_t i = 1; i < n; i++)
        if (c1_text(*shared[i]) != c1_text(*shared[0])) ok = false;
    cs.set_tensor_randomness(TensorRandomness::PerElement);
    auto t0 = Clock::now();
    auto ct = cs.encrypt_tensor(pk, pts);
    cs.synchronize();
    const double enc_ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    const bool enc_distinct = distinct_c1(ct), enc_dec = decrypts_to(ct, 1.0f);
    auto sum = cs.add_ciphertext_tensors(pk, ct, ct);
    Tensor<CS::PlainText *> three(n, nullptr);
    CS::PlainText p3 = cs.make_plaintext(3);
    for (size_t i = 0; i < n; i++) three.at(i) = &p3;
    auto tri = cs.scal_ciphertext_tensors(pk, three, ct);
    auto neg = cs.negate_ciphertext_tensor(pk, ct);
    t0 = Clock::now();
    auto rr = cs.rerandomize_ciphertext_tensor(pk, shared);
    cs.synchronize();
    const double rr_ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    const bool ops_distinct = distinct_c1(sum) && distinct_c1(tri) && distinct_c1(neg) && distinct_c1(rr);
    const bool ops_dec = decrypts_to(sum, 2.0f) && decrypts_to(tri, 3.0f) && decrypts_to(neg, -1.0f) && decrypts_to(rr, 1.0f);
    ok = ok && enc_distinct && enc_dec && ops_distinct && ops_dec;
    std::ofstream("local_bench_fresh_ct.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(ct);
    std::ofstream("local_bench_fresh_rerand.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(rr);
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    std::cout << "  per-element encrypt_tensor: " << enc_ms << " ms, rerandomize_ciphertext_tensor: " << rr_ms << " ms (" << n
              << " ciphertexts)" << std::endl;
    std::cout << "  distinct c1: encrypt " << (enc_distinct ? "yes" : "NO") << ", add / scal / negate / rerandomize "
              << (ops_distinct ? "yes" : "NO") << "; decryption: encrypt " << (enc_dec ? "yes" : "NO") << ", ops " << (ops_dec ? "yes" : "NO")
              << std::endl;
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    for (auto *t : {&shared, &ct, &sum, &tri, &neg, &rr}) free_all(*t);
    free_all(pts);
    if (!ok) throw std::runtime_error("fresh randomness check failed");
}

// differences and plaintext addends (sub_ciphertext_tensors, invert_ciphertext_tensor, add / sub_plaintext_tensor,
// plaintext_sub_ciphertext_tensor) against decryption, in the default mode, per element, 0-D and in PerElement mode
static void bench_affine(size_t n) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    Tensor<CS::PlainText *> pa(n, nullptr), pb(n, nullptr), pm(n, nullptr);
    std::vector<float> a(n), b(n), m(n);
    for (size_t i = 0; i < n; i++) {
        a[i] = (float)((long)(i * 7 % 101) - 50);
        b[i] = (float)((long)(i * 13 % 89) - 44);
        m[i] = (float)((long)(i * 5 % 61) - 30);
        pa.at(i) = new CS::PlainText(cs.make_plaintext(a[i]));
        pb.at(i) = new CS::PlainText(cs.make_plaintext(b[i]));
        pm.at(i) = new CS::PlainText(cs.make_plaintext(m[i]));
    }
    auto decrypts_to = [&](const Tensor<CS::CipherText *> &t, auto want) {
        auto res = cs.decrypt_tensor(sk, t);
        bool good = true;
        for (size_t i = 0; i < n; i++) {
            if (cs.get_float_from_plaintext(*res.at(i)) != want(i)) good = false;
            delete res.at(i);
        }
        return good;
    };
    auto c1_text = [](const CS::CipherText &c) { return c.c1().a().str() + " " + c.c1().b().str(); };
    auto distinct_c1 = [&](const Tensor<CS::CipherText *> &t) {
        std::set<std::string> seen;
        for (size_t i = 0; i < t.num_elements(); i++) seen.insert(c1_text(*t[i]));
        return seen.size() == t.num_elements();
    };
    auto ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
    cs.synchronize();
    bool ok = true;
    auto timed = [&](double &ms, auto fn) {
        auto t0 = Clock::now();
        auto r = fn();
        cs.synchronize();
        ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        return r;
    };
    double sub_ms = 0, neg_add_ms = 0, plain_ms = 0, enc_add_ms = 0;
    auto diff = timed(sub_ms, [&]() { return cs.sub_ciphertext_tensors(pk, ca, cb); });
    auto diff_ref = timed(neg_add_ms, [&]() {
        auto nb = cs.negate_ciphertext_tensor(pk, cb);
        auto r = cs.add_ciphertext_tensors(pk, ca, nb);
        free_all(nb);
        return r;
    });
    auto sum_m = timed(plain_ms, [&]() { return cs.add_plaintext_tensor(pk, ca, pm); });
    auto sum_ref = timed(enc_add_ms, [&]() {
        auto em = cs.encrypt_tensor(pk, pm);
        auto r = cs.add_ciphertext_tensors(pk, ca, em);
        free_all(em);
        return r;
    });
    auto dif_m = cs.sub_plaintext_tensor(pk, ca, pm);
    auto m_dif = cs.plaintext_sub_ciphertext_tensor(pk, pm, ca);
    auto inv = cs.invert_ciphertext_tensor(ca);
    const bool dec_ok = decrypts_to(diff, [&](size_t i) { return a[i] - b[i]; }) && decrypts_to(diff_ref, [&](size_t i) { return a[i] - b[i]; }) &&
                        decrypts_to(sum_m, [&](size_t i) { return a[i] + m[i]; }) && decrypts_to(sum_ref, [&](size_t i) { return a[i] + m[i]; }) &&
                        decrypts_to(dif_m, [&](size_t i) { return a[i] - m[i]; }) && decrypts_to(m_dif, [&](size_t i) { return m[i] - a[i]; }) &&
                        decrypts_to(inv, [&](size_t i) { return -a[i]; });
    // the plaintext addend leaves c1 alone: a tensor that shared its c1 still does
    bool c1_kept = true;
    for (size_t i = 0; i < n; i++)
        if (c1_text(*sum_m[i]) != c1_text(*ca[0]) || c1_text(*dif_m[i]) != c1_text(*ca[0])) c1_kept = false;
    // shape errors and the 0-D forms
    bool shape_ok = false;
    try {
        Tensor<CS::CipherText *> shorter(n > 1 ? n - 1 : 2, ca[0]);
        (void)cs.sub_ciphertext_tensors(pk, ca, shorter);
    } catch (const std::invalid_argument &e) {
        shape_ok = std::string(e.what()) == "Tensor shapes must be equal";
    }
    bool scalar_ok = true;
    {
        CS::CipherText x = *ca[1 % n], y = *cb[1 % n];
        CS::PlainText mm = *pm[1 % n];
        Tensor<CS::CipherText *> tx(&x), ty(&y);
        Tensor<CS::PlainText *> tm(&mm);
        auto d0 = cs.sub_ciphertext_tensors(pk, tx, ty);
        auto s0 = cs.add_plaintext_tensor(pk, tx, tm);
        auto i0 = cs.invert_ciphertext_tensor(tx);
        if (!d0.is_zero_degree() || !s0.is_zero_degree() || !i0.is_zero_degree()) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *d0.get_value())) != a[1 % n] - b[1 % n]) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *s0.get_value())) != a[1 % n] + m[1 % n]) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *i0.get_value())) != -a[1 % n]) scalar_ok = false;
        // the scalar difference is re-randomised like the scalar sum: a second call gives another ciphertext
        auto d1 = cs.sub_ciphertexts(pk, x, y);
        if (d1.c1() == d0.get_value()->c1()) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, d1)) != a[1 % n] - b[1 % n]) scalar_ok = false;
        delete d0.get_value(); delete s0.get_value(); delete i0.get_value();
    }
    std::ofstream("local_bench_affine_sub.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(diff);
    std::ofstream("local_bench_affine_plain.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(m_dif);
    // PerElement mode: the same results with a fresh r per element
    cs.set_tensor_randomness(TensorRandomness::PerElement);
    auto fdiff = cs.sub_ciphertext_tensors(pk, ca, cb);
    auto fsum = cs.add_plaintext_tensor(pk, ca, pm);
    auto fmdif = cs.plaintext_sub_ciphertext_tensor(pk, pm, ca);
    const bool fresh_ok = (n < 2 || (distinct_c1(fdiff) && distinct_c1(fsum) && distinct_c1(fmdif))) &&
                          decrypts_to(fdiff, [&](size_t i) { return a[i] - b[i]; }) && decrypts_to(fsum, [&](size_t i) { return a[i] + m[i]; }) &&
                          decrypts_to(fmdif, [&](size_t i) { return m[i] - a[i]; });
    cs.set_tensor_randomness(TensorRandomness::None);
    ok = dec_ok && c1_kept && shape_ok && scalar_ok && fresh_ok;
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    std::cout << "  sub_ciphertext_tensors " << sub_ms << " ms, negate + add " << neg_add_ms << " ms; add_plaintext_tensor " << plain_ms
              << " ms, encrypt_tensor + add " << enc_add_ms << " ms (" << n << " ciphertexts, host wall clock, first calls)" << std::endl;
    std::cout << "  decryption: " << (dec_ok ? "yes" : "NO") << ", c1 kept by the plaintext addend: " << (c1_kept ? "yes" : "NO")
              << ", shape error: " << (shape_ok ? "yes" : "NO") << ", 0-D forms: " << (scalar_ok ? "yes" : "NO") << ", per-element mode: "
              << (fresh_ok ? "yes" : "NO") << std::endl;
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    for (auto *t : {&ca, &cb, &diff, &diff_ref, &sum_m, &sum_ref, &dif_m, &m_dif, &inv, &fdiff, &fsum, &fmdif}) free_all(*t);
    free_all(pa); free_all(pb); free_all(pm);
    if (!ok) throw std::runtime_error("affine check failed");
}

// the Beaver element product with LocalCipherTextMultiplier::set_direct_differences: x*y mod 2^k as without it
static void bench_beaver_direct(size_t n) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    LocalSMPCClient<CS> client(cs, sk);
    LocalCipherTextMultiplier<CS> mul(client);
    const auto &pk = client.network_public_key();
    Tensor<CS::PlainText *> px(n, nullptr), py(n, nullptr);
    std::vector<float> want(n);
    for (size_t i = 0; i < n; i++) {
        const float x = (float)((long)(i % 7) - 3), y = (float)((long)(i % 5) + 1);
        want[i] = x * y;
        px.at(i) = new CS::PlainText(cs.make_plaintext(x));
        py.at(i) = new CS::PlainText(cs.make_plaintext(y));
    }
    auto cx = cs.encrypt_tensor(pk, px), cy = cs.encrypt_tensor(pk, py);
    bool ok = true;
    double ms[2] = {0, 0};
    for (int pass = 0; pass < 2; pass++)          // a warm-up pass builds the tables; the second is timed
        for (int direct = 0; direct < 2; direct++) {
            mul.set_direct_differences(direct != 0);
            cs.synchronize();
            auto t0 = Clock::now();
            auto res = mul.multiply_ciphertext_tensors(cx, cy);
            cs.synchronize();
            ms[direct] = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
            auto dec = cs.decrypt_tensor(sk, res);
            for (size_t i = 0; i < n; i++)
                if (cs.get_float_from_plaintext(*dec.at(i)) != want[i]) ok = false;
            if (direct && pass) std::ofstream("local_bench_beaver_direct.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(res);
            free_all(res);
            free_all(dec);
        }
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    std::cout << "  " << n << " element products: reference sequence " << ms[0] << " ms, direct differences " << ms[1]
              << " ms (host wall clock, triplet generation and decryptions included)" << std::endl;
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    free_all(cx); free_all(cy); free_all(px); free_all(py);
    if (!ok) throw std::runtime_error("beaver product mismatch");
}

// a polynomial activation on a ciphertext tensor from one opened value per element
// (LocalCipherTextMultiplier::evaluate_polynomial_ciphertext_tensor), through the single-key and the 2-of-3 threshold client:
// degree 3 with a negative coefficient over n elements, checked against p(x) mod 2^k from GMP on the host; prints
// client.decrypted_elements(), which must equal the element count
static void bench_poly_activation(size_t n, int runs) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    const uint32_t k = cs.message_bits();
    Mpz c[4] = {Mpz(5ul), Mpz(3ul), Mpz(7ul), Mpz(11ul)};
    c[1].neg();
    mpz_fdiv_r_2exp(c[1].get(), c[1].get(), k);                 // -3 mod 2^k
    Tensor<CS::PlainText *> coef(4, nullptr), px(n, nullptr);
    for (size_t j = 0; j < 4; j++) coef[j] = &c[j];
    std::vector<Mpz> want(n);
    for (size_t i = 0; i < n; i++) {
        // 0, 1, 2^k - 1, 2^(k-1), small values of both signs, then uniform ones
        Mpz x = i < 2 ? Mpz((unsigned long)i) : i < 8 ? cs.make_plaintext((float)((long)i - 5)) : cs.random_plaintext(k);
        if (i == 2 || i == 3) mpz_ui_pow_ui(x.get(), 2, i == 2 ? k : k - 1);
        if (i == 2) mpz_sub_ui(x.get(), x.get(), 1);
        for (int j = 3; j >= 0; j--) {                          // Horner mod 2^k
            mpz_mul(want[i].get(), want[i].get(), x.get());
            mpz_add(want[i].get(), want[i].get(), c[j].get());
            mpz_fdiv_r_2exp(want[i].get(), want[i].get(), k);
        }
        px[i] = new CS::PlainText(x);
    }
    bool ok = true;
    for (int threshold = 0; threshold < 2; threshold++) {
        std::unique_ptr<LocalSMPCClient<CS>> client(threshold ? new LocalSMPCClient<CS>(cs, sk, 2, 3) : new LocalSMPCClient<CS>(cs, sk));
        LocalCipherTextMultiplier<CS> mul(*client);
        auto cx = cs.encrypt_tensor(client->network_public_key(), px);
        cs.synchronize();
        auto t0 = Clock::now();
        auto res = mul.evaluate_polynomial_ciphertext_tensor(coef, cx);
        cs.synchronize();
        const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        auto dec = cs.decrypt_tensor(sk, res);
        bool pass = client->decrypted_elements() == n;
        for (size_t i = 0; i < n; i++)
            if (!(*dec.at(i) == want[i])) pass = false;
        if (!threshold) std::ofstream("local_bench_poly_activation.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(res);
        std::cout << "  " << (threshold ? "threshold 2 of 3" : "secret key") << ": degree 3 over " << n << " elements, decrypted_elements "
                  << client->decrypted_elements() << ", " << ms << " ms (host wall clock, tuple generation and the decryption included): "
                  << (pass ? "ok" : "FAILED") << std::endl;
        ok = ok && pass;
        free_all(res); free_all(dec);
        if (!threshold) {
            // the parts on their own: the square of the tensor and of one 0-D element, the Taylor shift (q_0 = p(x)), and the
            // two-base power product [x]^2 o [x]^3 = [5 x]
            const auto &pk = client->network_public_key();
            auto sq = mul.square_ciphertext_tensor(cx);
            auto sq0 = mul.square_ciphertext_tensor(Tensor<CS::CipherText *>(cx[1 % n]));
            auto dsq = cs.decrypt_tensor(sk, sq);
            auto dsq0 = cs.decrypt(sk, *sq0.get_value());
            auto q = cs.poly_shift_plaintext_tensor(coef, px);
            Mpz two(2ul), three(3ul);
            Vector<Tensor<CS::PlainText *>> exps{Tensor<CS::PlainText *>(n, &two), Tensor<CS::PlainText *>(n, &three)};
            Vector<Tensor<CS::CipherText *>> bases{cx, cx};
            auto dot = cs.pow_dot_ciphertext_tensors(pk, exps, bases);
            auto ddot = cs.decrypt_tensor(sk, dot);
            bool parts = q.size() == 4 && sq0.is_zero_degree();
            for (size_t i = 0; i < n; i++) {
                Mpz x2, x5;
                mpz_mul(x2.get(), px[i]->get(), px[i]->get());
                mpz_fdiv_r_2exp(x2.get(), x2.get(), k);
                mpz_mul_ui(x5.get(), px[i]->get(), 5);
                mpz_fdiv_r_2exp(x5.get(), x5.get(), k);
                if (!(*dsq.at(i) == x2) || !(*ddot.at(i) == x5) || !(*q[0].at(i) == want[i])) parts = false;
                if (i == 1 % n && !(dsq0 == x2)) parts = false;
            }
            std::cout << "  square (1-D and 0-D), poly_shift_plaintext_tensor, pow_dot_ciphertext_tensors: " << (parts ? "ok" : "FAILED") << std::endl;
            ok = ok && parts;
            delete sq0.get_value();
            free_all(sq); free_all(dsq); free_all(dot); free_all(ddot);
            for (auto &t : q) free_all(t);
        }
        free_all(cx);
    }
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    if (runs > 0) {
        // x^3 twice on the same input, single-key client: the polynomial (0, 0, 0, 1) with one opened value per element, and
        // (x * x) * x by two chained Beaver products with direct differences (four opened values per element, two rounds);
        // alternating, `runs` timed calls each after a warm-up of both; medians and extremes on one line for tools/bench_ops.py
        LocalSMPCClient<CS> client(cs, sk);
        LocalCipherTextMultiplier<CS> mul(client);
        mul.set_direct_differences(true);
        Mpz zero(0ul), one(1ul);
        Tensor<CS::PlainText *> cube(4, &zero);
        cube[3] = &one;
        auto cx = cs.encrypt_tensor(client.network_public_key(), px);
        std::vector<double> ms[2];
        size_t opened[2] = {0, 0};
        bool same = true;
        for (int pass = 0; pass <= runs; pass++)
            for (int chained = 0; chained < 2; chained++) {
                const size_t before = client.decrypted_elements();
                cs.synchronize();
                auto t0 = Clock::now();
                Tensor<CS::CipherText *> res;
                if (chained) {
                    auto sq = mul.multiply_ciphertext_tensors(cx, cx);
                    res = mul.multiply_ciphertext_tensors(sq, cx);
                    free_all(sq);
                } else {
                    res = mul.evaluate_polynomial_ciphertext_tensor(cube, cx);
                }
                cs.synchronize();
                if (pass) ms[chained].push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
                opened[chained] = client.decrypted_elements() - before;
                auto dec = cs.decrypt_tensor(sk, res);
                for (size_t i = 0; i < n; i++) {
                    Mpz w;
                    mpz_pow_ui(w.get(), px[i]->get(), 3);
                    mpz_fdiv_r_2exp(w.get(), w.get(), k);
                    if (!(*dec.at(i) == w)) same = false;
                }
                free_all(res); free_all(dec);
            }
        free_all(cx);
        for (auto &v : ms) std::sort(v.begin(), v.end());
        std::cout << "compare_json: {\"E\": " << n << ", \"degree\": 3, \"runs\": " << runs << ", \"poly_ms\": " << ms[0][ms[0].size() / 2]
                  << ", \"poly_ms_min_max\": [" << ms[0].front() << ", " << ms[0].back() << "], \"chained_products_ms\": " << ms[1][ms[1].size() / 2]
                  << ", \"chained_ms_min_max\": [" << ms[1].front() << ", " << ms[1].back() << "], \"chained_over_poly\": "
                  << ms[1][ms[1].size() / 2] / ms[0][ms[0].size() / 2] << ", \"opened_poly\": " << opened[0] << ", \"opened_chained\": " << opened[1]
                  << ", \"agree\": " << (same ? "true" : "false") << "}" << std::endl;
        ok = ok && same;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    free_all(px);
    if (!ok) throw std::runtime_error("polynomial activation mismatch");
}

// division of a ciphertext tensor by public divisors from one opened value per element
// (LocalCipherTextMultiplier::divide_ciphertext_tensor_by_plaintext), through the single-key and the 2-of-3 threshold client:
// a scalar divisor, a per-channel divisor (4 channels) and truncate by 2^16 over n elements with |x| < 2^40 of both signs (a
// wrap then has probability below 2^-80 per element at k = 128); every decrypted element must be floor(x / D) from GMP on the
// host or one less; prints client.decrypted_elements() per call, which must equal the element count.  runs > 0: the median
// wall clock of `runs` scalar divisions on one line for tools/bench_ops.py
static void bench_divide(size_t n, int runs) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    const uint32_t k = cs.message_bits();
    const size_t C = n % 4 == 0 ? 4 : 1;
    Tensor<CS::PlainText *> px(n, nullptr);
    std::vector<Mpz> xs(n);                                         // signed values
    for (size_t i = 0; i < n; i++) {
        // 0, 1, -1, the ends of the range, then uniform ones of both signs
        Mpz x = i < 2 ? Mpz((unsigned long)i) : cs.random_plaintext(40);
        if (i == 3 || i == 4) {
            mpz_set_ui(x.get(), 0);
            mpz_setbit(x.get(), 40);
            mpz_sub_ui(x.get(), x.get(), 1);
        }
        if (i == 2) mpz_set_ui(x.get(), 1);
        if (i == 2 || i == 4 || (i > 4 && i % 2)) x.neg();
        xs[i] = x;
        Mpz m;
        mpz_fdiv_r_2exp(m.get(), x.get(), k);
        px[i] = new CS::PlainText(m);
    }
    Mpz seven(7ul), per_channel[4] = {Mpz(3ul), Mpz(1000003ul), Mpz(1ul), Mpz(2ul)};
    mpz_mul_2exp(per_channel[1].get(), per_channel[1].get(), 20);   // beyond one limb
    Tensor<CS::PlainText *> dscalar(1, &seven), dchan(C, nullptr);
    for (size_t c = 0; c < C; c++) dchan[c] = &per_channel[c];
    const uint32_t t_bits = 16;
    // res decrypts to floor(x / D) or one less, as residues mod 2^k
    auto agrees = [&](const Tensor<CS::PlainText *> &dec, const Tensor<CS::PlainText *> &div) {
        bool pass = true;
        for (size_t i = 0; i < n; i++) {
            Mpz q, q1, a, b;
            mpz_fdiv_q(q.get(), xs[i].get(), div[i % div.num_elements()]->get());
            mpz_sub_ui(q1.get(), q.get(), 1);
            mpz_fdiv_r_2exp(a.get(), q.get(), k);
            mpz_fdiv_r_2exp(b.get(), q1.get(), k);
            if (!(*dec.at(i) == a) && !(*dec.at(i) == b)) pass = false;
        }
        return pass;
    };
    bool ok = true;
    for (int threshold = 0; threshold < 2; threshold++) {
        std::unique_ptr<LocalSMPCClient<CS>> client(threshold ? new LocalSMPCClient<CS>(cs, sk, 2, 3) : new LocalSMPCClient<CS>(cs, sk));
        LocalCipherTextMultiplier<CS> mul(*client);
        auto cx = cs.encrypt_tensor(client->network_public_key(), px);
        Mpz two_t;
        mpz_setbit(two_t.get(), t_bits);
        Tensor<CS::PlainText *> dtrunc(1, &two_t);
        const char *names[3] = {"scalar divisor 7", "per-channel divisors", "truncate by 2^16"};
        for (int what = 0; what < 3; what++) {
            const size_t before = client->decrypted_elements();
            cs.synchronize();
            auto t0 = Clock::now();
            auto res = what == 0 ? mul.divide_ciphertext_tensor_by_plaintext(cx, dscalar)
                       : what == 1 ? mul.divide_ciphertext_tensor_by_plaintext(cx, dchan)
                                   : mul.truncate_ciphertext_tensor(cx, t_bits);
            cs.synchronize();
            const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
            const size_t opened = client->decrypted_elements() - before;
            auto dec = cs.decrypt_tensor(sk, res);
            const bool pass = opened == n && agrees(dec, what == 0 ? dscalar : what == 1 ? dchan : dtrunc);
            if (!threshold && what == 0) std::ofstream("local_bench_divide.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(res);
            std::cout << "  " << (threshold ? "threshold 2 of 3" : "secret key") << ": " << names[what] << " over " << n << " elements, opened_values "
                      << opened << ", " << ms << " ms (host wall clock, pair generation and the decryption included): " << (pass ? "ok" : "FAILED")
                      << std::endl;
            ok = ok && pass;
            free_all(res); free_all(dec);
        }
        if (!threshold) {
            // the parts on their own: one 0-D element, the plaintext division, an invalid divisor, and the mean of 2 x 2 windows
            auto q0 = mul.divide_ciphertext_tensor_by_plaintext(Tensor<CS::CipherText *>(cx[2 % n]), Tensor<CS::PlainText *>(&seven));
            auto dq0 = cs.decrypt(sk, *q0.get_value());
            auto pq = cs.divide_plaintext_tensor(px, dscalar);
            bool parts = q0.is_zero_degree();
            for (size_t i = 0; i < n; i++) {
                Mpz q, a, b;
                mpz_fdiv_q(q.get(), xs[i].get(), seven.get());
                mpz_fdiv_r_2exp(a.get(), q.get(), k);
                mpz_sub_ui(q.get(), q.get(), 1);
                mpz_fdiv_r_2exp(b.get(), q.get(), k);
                if (!(*pq.at(i) == a)) parts = false;
                if (i == 2 % n && !(dq0 == a) && !(dq0 == b)) parts = false;
            }
            Mpz zero(0ul);
            bool refused = false;
            try {
                (void)mul.divide_ciphertext_tensor_by_plaintext(cx, Tensor<CS::PlainText *>(1, &zero));
            } catch (const std::invalid_argument &) {
                refused = true;
            }
            parts = parts && refused;
            if (n % 4 == 0) {
                Tensor<CS::CipherText *> img = cx;
                img.reshape({1, 2, 2, n / 4});
                auto avg = mul.avg_pool2d_ciphertext_tensor(img, {2, 2}, {2, 2});
                auto davg = cs.decrypt_tensor(sk, avg);
                for (size_t c = 0; c < n / 4; c++) {
                    Mpz s, q, a, b;
                    for (size_t p = 0; p < 4; p++) mpz_add(s.get(), s.get(), xs[p * (n / 4) + c].get());
                    mpz_fdiv_q_ui(q.get(), s.get(), 4);
                    mpz_fdiv_r_2exp(a.get(), q.get(), k);
                    mpz_sub_ui(q.get(), q.get(), 1);
                    mpz_fdiv_r_2exp(b.get(), q.get(), k);
                    if (!(*davg[c] == a) && !(*davg[c] == b)) parts = false;
                }
                free_all(avg); free_all(davg);
            }
            std::cout << "  0-D division, divide_plaintext_tensor, the refusal of divisor 0, avg_pool2d: " << (parts ? "ok" : "FAILED") << std::endl;
            ok = ok && parts;
            delete q0.get_value();
            free_all(pq);
        }
        free_all(cx);
    }
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    if (runs > 0) {
        LocalSMPCClient<CS> client(cs, sk);
        LocalCipherTextMultiplier<CS> mul(client);
        auto cx = cs.encrypt_tensor(client.network_public_key(), px);
        std::vector<double> ms;
        for (int pass = 0; pass <= runs; pass++) {
            cs.synchronize();
            auto t0 = Clock::now();
            auto res = mul.divide_ciphertext_tensor_by_plaintext(cx, dscalar);
            cs.synchronize();
            if (pass) ms.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
            free_all(res);
        }
        free_all(cx);
        std::sort(ms.begin(), ms.end());
        std::cout << "divide_json: {\"E\": " << n << ", \"runs\": " << runs << ", \"divide_ms\": " << ms[ms.size() / 2] << ", \"divide_ms_min_max\": ["
                  << ms.front() << ", " << ms.back() << "]}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    free_all(px);
    if (!ok) throw std::runtime_error("division mismatch");
}

// table lookups on a ciphertext tensor from one opened value per element (LocalCipherTextMultiplier::lookup_ciphertext_tensor),
// through the single-key and the 2-of-3 threshold client: a random 8-bit table, relu and max at 8 bits over n elements of the
// whole signed 8-bit range, and a 2 x 2 max pool of them (n a multiple of 4); every decrypted element must EQUAL the plaintext
// computation; prints the opened values per call (n for a lookup, 3 per output for the 2 x 2 pool) and whether all c1 of one
// tuple tensor are pairwise distinct in the default randomness mode.  runs > 0: the median wall clock of `runs` relu calls on
// one line for tools/bench_ops.py
static void bench_lookup(size_t n, int runs) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    const uint32_t k = cs.message_bits(), bits = 8;
    const long half = 1L << (bits - 1);
    // signed values: the ends of the range, 0, -1, 1, then uniform ones
    std::vector<long> xs(n), ys(n);
    const long fixed[5] = {-half, half - 1, 0, -1, 1};
    for (size_t i = 0; i < n; i++) {
        xs[i] = i < 5 ? fixed[i] : (long)mpz_get_ui(cs.random_plaintext(bits).get()) - half;
        ys[i] = i < 5 ? fixed[4 - i] : (long)mpz_get_ui(cs.random_plaintext(bits).get()) - half;
    }
    auto residue = [&](long v) {                                    // v mod 2^k
        Mpz m((unsigned long)(v < 0 ? -v : v));
        if (v < 0) m.neg();
        mpz_fdiv_r_2exp(m.get(), m.get(), k);
        return m;
    };
    auto plain = [&](const std::vector<long> &v) {
        Tensor<CS::PlainText *> t(v.size(), nullptr);
        for (size_t i = 0; i < v.size(); i++) t[i] = new CS::PlainText(residue(v[i]));
        return t;
    };
    auto px = plain(xs), py = plain(ys);
    std::vector<Mpz> g((size_t)1 << bits);                          // any public function: 256 uniform k-bit plaintexts
    Tensor<CS::PlainText *> table(g.size(), nullptr);
    for (size_t j = 0; j < g.size(); j++) {
        g[j] = cs.random_plaintext(k);
        table[j] = &g[j];
    }
    auto equals = [&](const Tensor<CS::PlainText *> &dec, const std::vector<Mpz> &want) {
        bool pass = dec.num_elements() == want.size();
        for (size_t i = 0; pass && i < want.size(); i++) pass = *dec[i] == want[i];
        return pass;
    };
    bool ok = true;
    for (int threshold = 0; threshold < 2; threshold++) {
        std::unique_ptr<LocalSMPCClient<CS>> client(threshold ? new LocalSMPCClient<CS>(cs, sk, 2, 3) : new LocalSMPCClient<CS>(cs, sk));
        LocalCipherTextMultiplier<CS> mul(*client);
        auto cx = cs.encrypt_tensor(client->network_public_key(), px), cy = cs.encrypt_tensor(client->network_public_key(), py);
        const char *who = threshold ? "threshold 2 of 3" : "secret key";
        const char *names[3] = {"random 8-bit table", "relu at 8 bits", "max at 8 bits"};
        for (int what = 0; what < 3; what++) {
            std::vector<Mpz> want(n);
            for (size_t i = 0; i < n; i++)
                want[i] = what == 0 ? g[(size_t)(xs[i] & ((1L << bits) - 1))] : residue(what == 1 ? std::max(xs[i], 0L) : std::max(xs[i], ys[i]));
            const size_t before = client->decrypted_elements();
            cs.synchronize();
            auto t0 = Clock::now();
            auto res = what == 0 ? mul.lookup_ciphertext_tensor(table, cx) : what == 1 ? mul.relu_ciphertext_tensor(cx, bits)
                                                                                       : mul.max_ciphertext_tensors(cx, cy, bits);
            cs.synchronize();
            const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
            const size_t opened = client->decrypted_elements() - before;
            auto dec = cs.decrypt_tensor(sk, res);
            const bool pass = opened == n && equals(dec, want);
            if (!threshold && what == 1) std::ofstream("local_bench_lookup.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(res);
            std::cout << "  " << who << ": " << names[what] << " over " << n << " elements, opened_values " << opened << ", " << ms
                      << " ms (host wall clock, tuple generation and the decryption included): " << (pass ? "ok" : "FAILED") << std::endl;
            ok = ok && pass;
            free_all(res); free_all(dec);
        }
        if (n % 4 == 0) {
            Tensor<CS::CipherText *> img = cx;
            img.reshape({1, 2, 2, n / 4});
            const size_t before = client->decrypted_elements();
            auto pooled = mul.max_pool2d_ciphertext_tensor(img, {2, 2}, {2, 2}, bits);
            const size_t opened = client->decrypted_elements() - before;
            auto dec = cs.decrypt_tensor(sk, pooled);
            std::vector<Mpz> want(n / 4);
            for (size_t c = 0; c < n / 4; c++) {
                long m = xs[c];
                for (size_t p = 1; p < 4; p++) m = std::max(m, xs[p * (n / 4) + c]);
                want[c] = residue(m);
            }
            const bool pass = opened == 3 * (n / 4) && equals(dec, want);
            std::cout << "  " << who << ": 2 x 2 max pool, opened_values " << opened << " for " << n / 4 << " outputs, two rounds: " << (pass ? "ok" : "FAILED")
                      << std::endl;
            ok = ok && pass;
            free_all(pooled); free_all(dec);
        }
        if (!threshold) {
            // the parts on their own: one 0-D element, the plaintext rows, the refusals, and the randomness of a tuple tensor
            auto y0 = mul.lookup_ciphertext_tensor(table, Tensor<CS::CipherText *>(cx[1 % n]));
            bool parts = y0.is_zero_degree() && cs.decrypt(sk, *y0.get_value()) == g[(size_t)(xs[1 % n] & ((1L << bits) - 1))];
            delete y0.get_value();
            Mpz three(3ul);
            auto rows = cs.lut_rotate_plaintext_tensor(table, Tensor<CS::PlainText *>(1, &three));
            for (size_t j = 0; j < g.size(); j++) parts = parts && *rows[j] == g[(j + 3) % g.size()];
            free_all(rows);
            int refused = 0;
            try {
                (void)mul.lookup_ciphertext_tensor(Tensor<CS::PlainText *>(3, &three), cx);       // 3 entries: no power of two
            } catch (const std::invalid_argument &) {
                refused++;
            }
            try {
                (void)mul.relu_ciphertext_tensor(cx, 13);
            } catch (const std::invalid_argument &) {
                refused++;
            }
            parts = parts && refused == 2;
            std::cout << "  0-D lookup, lut_rotate_plaintext_tensor, the refusals of 3 entries and of 13 bits: " << (parts ? "ok" : "FAILED") << std::endl;
            ok = ok && parts;
            const bool default_mode = cs.tensor_randomness() == TensorRandomness::None;
            auto tuples = client->get_lookup_tuples(4, table);
            std::set<std::string> seen;
            for (auto &t : tuples)
                for (size_t i = 0; i < t.num_elements(); i++) seen.insert(t[i]->c1().a().str() + " " + t[i]->c1().b().str());
            const bool distinct = default_mode && seen.size() == 4 + 4 * g.size();
            std::cout << "  " << 4 + 4 * g.size() << " ciphertexts of the tuples of 4 elements, default randomness mode, distinct c1: "
                      << (distinct ? "yes" : "NO") << std::endl;
            ok = ok && distinct;
            for (auto &t : tuples) free_all(t);
        }
        free_all(cx); free_all(cy);
    }
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    if (runs > 0) {
        LocalSMPCClient<CS> client(cs, sk);
        LocalCipherTextMultiplier<CS> mul(client);
        auto cx = cs.encrypt_tensor(client.network_public_key(), px);
        std::vector<double> ms;
        for (int pass = 0; pass <= runs; pass++) {
            cs.synchronize();
            auto t0 = Clock::now();
            auto res = mul.relu_ciphertext_tensor(cx, bits);
            cs.synchronize();
            if (pass) ms.push_back(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
            free_all(res);
        }
        free_all(cx);
        std::sort(ms.begin(), ms.end());
        std::cout << "lookup_json: {\"E\": " << n << ", \"bits\": " << bits << ", \"runs\": " << runs << ", \"relu_ms\": " << ms[ms.size() / 2]
                  << ", \"relu_ms_min_max\": [" << ms.front() << ", " << ms.back() << "]}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    free_all(px); free_all(py);
    if (!ok) throw std::runtime_error("lookup mismatch");
}

// threshold decryption end to end (the reference has no local benchmark for it; the calls are the
// ones PartialDecryptionRequestHandler / SMPCClient make, partial_decryption_request_handler.hpp:140,
// smpc_client.hpp:137): share sk t-out-of-n, every party of the first threshold set runs
// part_decrypt_tensor, the combiner runs combine_part_decryption_results_tensor.
static void bench_threshold(size_t n, size_t m, size_t t, size_t parties) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    auto shares = cs.keygen(sk, t, parties);
    // host check of the sharing: for the first threshold set {0..t-1}, s_0 - s_1 - ... - s_(t-1) = sk
    {
        Mpz acc = shares[0][0];
        for (size_t j = 1; j < t; j++) mpz_sub(acc.get(), acc.get(), shares[j][0].get());
        if (!(acc == sk)) throw std::runtime_error("shares do not reconstruct the secret key");
    }
    Tensor<CS::PlainText *> pts(n, m, nullptr);
    pts.flatten();
    for (size_t i = 0; i < n * m; i++) pts.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
    pts.reshape({n, m});
    auto ct = cs.encrypt_tensor(pk, pts);
    Benchmark bp("part_decrypt_tensor"), bc("combine_part_decryption_results_tensor");
    Vector<Tensor<CS::PartDecryptionResult *>> pdrs;
    bp.run([&]() { pdrs.push_back(cs.part_decrypt_tensor(shares[pdrs.size()][0], ct)); }, (int)t);
    // wire format round trip of the first party's result
    {
        auto bytes = cs.serialize_part_decryption_result_tensor(pdrs[0]);
        auto back = cs.deserialize_part_decryption_result_tensor(bytes);
        if (cs.serialize_part_decryption_result_tensor(back) != bytes) throw std::runtime_error("pdr format round trip");
        free_all(back);
    }
    bool ok = true;
    bc.run([&]() {
        auto res = cs.combine_part_decryption_results_tensor(ct, pdrs);
        res.flatten();
        for (size_t i = 0; i < res.num_elements(); i++) {
            if (cs.get_float_from_plaintext(*res.at(i)) != (float)(i + 1)) ok = false;
            delete res.at(i);
        }
    }, 1);
    bp.print_summary();
    bc.print_summary();
    for (auto &p : pdrs) free_all(p);
    free_all(ct);
    free_all(pts);
    std::cout << "  threshold " << t << " of " << parties << ": " << (ok ? "ok" : "FAILED") << std::endl;
    std::cout << "n: " << n << " m: " << m << std::endl;
    if (!ok) throw std::runtime_error("threshold decryption mismatch");
}

// ciphertext x ciphertext matrix product through the Beaver-triplet protocol with an in-process
// client (smpc_local.hpp; reference: SMPCCipherTextMultiplier::multiply_ciphertext_tensors,
// include/smpc/ciphertext_multiplications.hpp:40-112).  threshold = 0: the client decrypts with the
// secret key; otherwise by t-of-n threshold decryption.
static void bench_ciphertext_matmul(size_t n, size_t m, size_t p, size_t t, size_t parties) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    std::unique_ptr<LocalSMPCClient<CS>> client(t ? new LocalSMPCClient<CS>(cs, sk, t, parties) : new LocalSMPCClient<CS>(cs, sk));
    LocalCipherTextMultiplier<CS> mul(*client);
    const auto &pk = client->network_public_key();
    Tensor<CS::PlainText *> pa(n, m, nullptr), pb(m, p, nullptr);
    pa.flatten(); pb.flatten();
    for (size_t i = 0; i < n * m; i++) pa.at(i) = new CS::PlainText(cs.make_plaintext((float)(i % 7) - 3.0f));
    for (size_t i = 0; i < m * p; i++) pb.at(i) = new CS::PlainText(cs.make_plaintext((float)(i % 5) + 1.0f));
    pa.reshape({n, m}); pb.reshape({m, p});
    auto ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
    Benchmark b("ciphertext_matmul (Beaver triplets, in-process client)");
    bool ok = true;
    b.run([&]() {
        auto res = mul.multiply_ciphertext_tensors(ca, cb);
        auto dec = cs.decrypt_tensor(sk, res);
        res.flatten(); dec.flatten();
        for (size_t i = 0; i < n; i++)
            for (size_t k = 0; k < p; k++) {
                float want = 0;
                for (size_t j = 0; j < m; j++) want += ((float)((i * m + j) % 7) - 3.0f) * ((float)((j * p + k) % 5) + 1.0f);
                if (cs.get_float_from_plaintext(*dec.at(i * p + k)) != want) ok = false;
            }
        free_all(res);
        free_all(dec);
    }, 1);
    b.print_summary();
    std::cout << "  " << n * m * p << " element products, " << client->decrypted_elements() << " decryptions"
              << (t ? " (threshold " + std::to_string(t) + " of " + std::to_string(parties) + ")" : std::string(" (secret key)"))
              << ": " << (ok ? "ok" : "FAILED") << std::endl;
    std::cout << "n: " << n << " m: " << m << " p: " << p << std::endl;
    free_all(ca); free_all(cb); free_all(pa); free_all(pb);
    if (!ok) throw std::runtime_error("ciphertext matmul mismatch");
}

// plaintext matrix (n x m) . ciphertext matrix (m x p), the linear layer y = W x: deterministic operands and a fixed Enc(0),
// written to files for the parity checker like the scal_matmul mode (local_bench_lmm_*.bin)
static void bench_plain_ct_matmul(size_t n, size_t m, size_t p) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    Tensor<CS::PlainText *> w(n, m, nullptr), x(m, p, nullptr);
    for (size_t i = 0; i < n * m; i++) w[i] = new CS::PlainText(cs.make_plaintext((float)(i % 7) - 3.0f));       // weights of both signs
    for (size_t i = 0; i < m * p; i++) x[i] = new CS::PlainText(cs.make_plaintext((float)(i + 1)));
    auto cx = cs.encrypt_tensor(pk, x);
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    Benchmark b("plain_ct_matmul (plaintext n x m . ciphertext m x p)");
    std::string out_bytes;
    bool ok = true;
    b.run([&]() {
        auto res = cs.matmul_plaintext_ciphertext_tensors(pk, w, cx, &zero);
        out_bytes = cs.serialize_ciphertext_tensor(res);
        auto dec = cs.decrypt_tensor(sk, res);
        for (size_t i = 0; i < n; i++)
            for (size_t k = 0; k < p; k++) {
                float want = 0;
                for (size_t j = 0; j < m; j++) want += ((float)((i * m + j) % 7) - 3.0f) * (float)(j * p + k + 1);
                if (cs.get_float_from_plaintext(*dec[i * p + k]) != want) ok = false;
            }
        free_all(res);
        free_all(dec);
    }, 1);
    b.print_summary();
    std::ofstream("local_bench_lmm_s.bin", std::ios::binary) << cs.serialize_plaintext_tensor(w);
    std::ofstream("local_bench_lmm_cts.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(cx);
    {
        Tensor<CS::CipherText *> zt(1, &zero);
        std::ofstream("local_bench_lmm_zero.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(zt);
    }
    std::ofstream("local_bench_lmm_out.bin", std::ios::binary) << out_bytes;
    {
        Mpz ad = cs.discriminant();
        ad.neg();
        std::ofstream("local_bench_absdelta.txt") << ad.str() << "\n";
    }
    free_all(w); free_all(x); free_all(cx);
    std::cout << "  decrypts to W x: " << (ok ? "yes" : "NO") << std::endl;
    std::cout << "n: " << n << " m: " << m << " p: " << p << std::endl;
    if (!ok) throw std::runtime_error("plaintext-left product mismatch");
}

// plaintext filters kh x kw x C x Co over an encrypted image B x H x W x C (channels last): encrypt, convolve, decrypt and
// compare with the convolution of the plaintexts
static void bench_conv2d(size_t B, size_t H, size_t W, size_t C, size_t kh, size_t kw, size_t Co, size_t sh, size_t sw, size_t ph, size_t pw) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    auto xval = [](size_t i) { return (float)(i % 11) - 4.0f; };
    auto wval = [](size_t i) { return (float)(i % 7) - 3.0f; };               // weights of both signs, zeros among them
    Tensor<CS::PlainText *> x({B, H, W, C}, nullptr), w({kh, kw, C, Co}, nullptr);
    for (size_t i = 0; i < x.num_elements(); i++) x[i] = new CS::PlainText(cs.make_plaintext(xval(i)));
    for (size_t i = 0; i < w.num_elements(); i++) w[i] = new CS::PlainText(cs.make_plaintext(wval(i)));
    auto cx = cs.encrypt_tensor(pk, x);
    Benchmark b("conv2d (plaintext filters over a ciphertext image)");
    bool ok = true;
    std::vector<size_t> oshape;
    b.run([&]() {
        auto res = cs.conv2d_plaintext_ciphertext_tensors(pk, w, cx, {sh, sw}, {ph, pw});
        oshape = res.shape();
        auto dec = cs.decrypt_tensor(sk, res);
        const size_t Ho = oshape[1], Wo = oshape[2];
        for (size_t bb = 0; bb < B; bb++)
            for (size_t oy = 0; oy < Ho; oy++)
                for (size_t ox = 0; ox < Wo; ox++)
                    for (size_t co = 0; co < Co; co++) {
                        float want = 0;
                        for (size_t dy = 0; dy < kh; dy++)
                            for (size_t dx = 0; dx < kw; dx++) {
                                const size_t y = oy * sh + dy, xx = ox * sw + dx;
                                if (y < ph || y - ph >= H || xx < pw || xx - pw >= W) continue;
                                for (size_t ci = 0; ci < C; ci++)
                                    want += xval(((bb * H + (y - ph)) * W + (xx - pw)) * C + ci) * wval(((dy * kw + dx) * C + ci) * Co + co);
                            }
                        if (cs.get_float_from_plaintext(*dec[((bb * Ho + oy) * Wo + ox) * Co + co]) != want) ok = false;
                    }
        free_all(res);
        free_all(dec);
    }, 1);
    b.print_summary();
    free_all(x); free_all(w); free_all(cx);
    if (oshape.size() != 4 || oshape[0] != B || oshape[3] != Co) ok = false;
    std::cout << "  decrypts to the convolution: " << (ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << B << "x" << H << "x" << W << "x" << C << " filters: " << kh << "x" << kw << "x" << C << "x" << Co << " stride: " << sh << "," << sw
              << " pad: " << ph << "," << pw << " out: " << (oshape.size() == 4 ? oshape[1] : 0) << "x" << (oshape.size() == 4 ? oshape[2] : 0) << std::endl;
    if (!ok) throw std::runtime_error("convolution mismatch");
}

// the same with dilation and groups: filters kh x kw x C/G x Co, output column co reads the channels of group co / (Co / G)
static void bench_conv2d_grouped(size_t B, size_t H, size_t W, size_t C, size_t kh, size_t kw, size_t Co, size_t G, size_t dh, size_t dw, size_t sh,
                                 size_t sw, size_t ph, size_t pw) {
    if (G == 0 || C % G || Co % G) throw std::invalid_argument("conv2d_grouped: groups must divide C and Co");
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    const size_t Cg = C / G, Cog = Co / G;
    auto xval = [](size_t i) { return (float)(i % 11) - 4.0f; };
    auto wval = [](size_t i) { return (float)(i % 7) - 3.0f; };               // weights of both signs, zeros among them
    Tensor<CS::PlainText *> x({B, H, W, C}, nullptr), w({kh, kw, Cg, Co}, nullptr);
    for (size_t i = 0; i < x.num_elements(); i++) x[i] = new CS::PlainText(cs.make_plaintext(xval(i)));
    for (size_t i = 0; i < w.num_elements(); i++) w[i] = new CS::PlainText(cs.make_plaintext(wval(i)));
    auto cx = cs.encrypt_tensor(pk, x);
    Benchmark b("conv2d_grouped (plaintext filters in groups over a ciphertext image)");
    bool ok = true;
    std::vector<size_t> oshape;
    b.run([&]() {
        auto res = cs.conv2d_plaintext_ciphertext_tensors(pk, w, cx, {sh, sw}, {ph, pw}, {dh, dw}, G);
        oshape = res.shape();
        auto dec = cs.decrypt_tensor(sk, res);
        const size_t Ho = oshape[1], Wo = oshape[2];
        for (size_t bb = 0; bb < B; bb++)
            for (size_t oy = 0; oy < Ho; oy++)
                for (size_t ox = 0; ox < Wo; ox++)
                    for (size_t co = 0; co < Co; co++) {
                        float want = 0;
                        for (size_t dy = 0; dy < kh; dy++)
                            for (size_t dx = 0; dx < kw; dx++) {
                                const size_t y = oy * sh + dy * dh, xx = ox * sw + dx * dw;
                                if (y < ph || y - ph >= H || xx < pw || xx - pw >= W) continue;
                                for (size_t ci = 0; ci < Cg; ci++)
                                    want += xval(((bb * H + (y - ph)) * W + (xx - pw)) * C + (co / Cog) * Cg + ci) * wval(((dy * kw + dx) * Cg + ci) * Co + co);
                            }
                        if (cs.get_float_from_plaintext(*dec[((bb * Ho + oy) * Wo + ox) * Co + co]) != want) ok = false;
                    }
        free_all(res);
        free_all(dec);
    }, 1);
    b.print_summary();
    free_all(x); free_all(w); free_all(cx);
    if (oshape.size() != 4 || oshape[0] != B || oshape[3] != Co) ok = false;
    std::cout << "  decrypts to the grouped convolution: " << (ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << B << "x" << H << "x" << W << "x" << C << " filters: " << kh << "x" << kw << "x" << Cg << "x" << Co << " groups: " << G
              << " dilation: " << dh << "," << dw << " stride: " << sh << "," << sw << " pad: " << ph << "," << pw
              << " out: " << (oshape.size() == 4 ? oshape[1] : 0) << "x" << (oshape.size() == 4 ? oshape[2] : 0) << std::endl;
    if (!ok) throw std::runtime_error("grouped convolution mismatch");
}

// sum pooling over kh x kw windows of an encrypted image B x H x W x C: encrypt, pool, decrypt and compare with the window sums
static void bench_sum_pool2d(size_t B, size_t H, size_t W, size_t C, size_t kh, size_t kw, size_t sh, size_t sw, size_t ph, size_t pw) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    auto xval = [](size_t i) { return (float)(i % 11) - 4.0f; };
    Tensor<CS::PlainText *> x({B, H, W, C}, nullptr);
    for (size_t i = 0; i < x.num_elements(); i++) x[i] = new CS::PlainText(cs.make_plaintext(xval(i)));
    auto cx = cs.encrypt_tensor(pk, x);
    Benchmark b("sum_pool2d (window sums of a ciphertext image)");
    bool ok = true;
    std::vector<size_t> oshape;
    b.run([&]() {
        auto res = cs.sum_pool2d_ciphertext_tensor(pk, cx, {kh, kw}, {sh, sw}, {ph, pw});
        oshape = res.shape();
        auto dec = cs.decrypt_tensor(sk, res);
        const size_t Ho = oshape[1], Wo = oshape[2];
        for (size_t bb = 0; bb < B; bb++)
            for (size_t oy = 0; oy < Ho; oy++)
                for (size_t ox = 0; ox < Wo; ox++)
                    for (size_t c = 0; c < C; c++) {
                        float want = 0;
                        for (size_t dy = 0; dy < kh; dy++)
                            for (size_t dx = 0; dx < kw; dx++) {
                                const size_t y = oy * sh + dy, xx = ox * sw + dx;
                                if (y < ph || y - ph >= H || xx < pw || xx - pw >= W) continue;
                                want += xval(((bb * H + (y - ph)) * W + (xx - pw)) * C + c);
                            }
                        if (cs.get_float_from_plaintext(*dec[((bb * Ho + oy) * Wo + ox) * C + c]) != want) ok = false;
                    }
        free_all(res);
        free_all(dec);
    }, 1);
    b.print_summary();
    free_all(x); free_all(cx);
    if (oshape.size() != 4 || oshape[0] != B || oshape[3] != C) ok = false;
    std::cout << "  decrypts to the window sums: " << (ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << B << "x" << H << "x" << W << "x" << C << " window: " << kh << "x" << kw << " stride: " << sh << "," << sw << " pad: " << ph << ","
              << pw << " out: " << (oshape.size() == 4 ? oshape[1] : 0) << "x" << (oshape.size() == 4 ? oshape[2] : 0) << std::endl;
    if (!ok) throw std::runtime_error("sum pooling mismatch");
}

// the ciphertext x ciphertext matrix product twice on the same inputs: the reference's expansion into n m p element
// products (2 n m p opened values) and one matrix triplet (LocalCipherTextMultiplier::set_matrix_triplets: n m + m p)
static void bench_ciphertext_matmul_matrix(size_t n, size_t m, size_t p, size_t t, size_t parties) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    std::unique_ptr<LocalSMPCClient<CS>> client(t ? new LocalSMPCClient<CS>(cs, sk, t, parties) : new LocalSMPCClient<CS>(cs, sk));
    LocalCipherTextMultiplier<CS> mul(*client);
    const auto &pk = client->network_public_key();
    Tensor<CS::PlainText *> pa(n, m, nullptr), pb(m, p, nullptr);
    for (size_t i = 0; i < n * m; i++) pa[i] = new CS::PlainText(cs.make_plaintext((float)(i % 7) - 3.0f));
    for (size_t i = 0; i < m * p; i++) pb[i] = new CS::PlainText(cs.make_plaintext((float)(i % 5) + 1.0f));
    auto ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
    bool ok[2] = {true, true};
    double ms[2] = {0, 0};
    size_t opened[2] = {0, 0};
    for (int matrix = 0; matrix < 2; matrix++) {
        mul.set_matrix_triplets(matrix != 0);
        const size_t before = client->decrypted_elements();
        cs.synchronize();
        auto t0 = Clock::now();
        auto res = mul.multiply_ciphertext_tensors(ca, cb);
        cs.synchronize();
        ms[matrix] = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        opened[matrix] = client->decrypted_elements() - before;
        auto dec = cs.decrypt_tensor(sk, res);
        for (size_t i = 0; i < n; i++)
            for (size_t k = 0; k < p; k++) {
                float want = 0;
                for (size_t j = 0; j < m; j++) want += ((float)((i * m + j) % 7) - 3.0f) * ((float)((j * p + k) % 5) + 1.0f);
                if (cs.get_float_from_plaintext(*dec[i * p + k]) != want) ok[matrix] = false;
            }
        free_all(res);
        free_all(dec);
    }
    const std::string how = t ? "threshold " + std::to_string(t) + " of " + std::to_string(parties) : std::string("secret key");
    std::cout << "  element flow: decrypted_elements " << opened[0] << ", " << ms[0] << " ms: " << (ok[0] ? "ok" : "FAILED") << std::endl;
    std::cout << "  matrix flow: decrypted_elements " << opened[1] << ", " << ms[1] << " ms: " << (ok[1] ? "ok" : "FAILED") << std::endl;
    std::cout << "  (host wall clock, triplet generation and decryptions included; " << how << ")" << std::endl;
    std::cout << "  agree: " << (ok[0] && ok[1] ? "yes" : "NO") << std::endl;
    std::cout << "n: " << n << " m: " << m << " p: " << p << std::endl;
    free_all(ca); free_all(cb); free_all(pa); free_all(pb);
    if (!(ok[0] && ok[1])) throw std::runtime_error("ciphertext matmul mismatch");
}

// text formats of single values and the binary plaintext-tensor format (cpu_cryptosystem.inl:124-318): written to
// files for the parity checker, and read back
static void bench_formats() {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    auto ct = cs.encrypt(pk, cs.make_plaintext(42));
    bool ok = true;
    const std::string txt = cs.serialize_ciphertext(ct);
    auto back = cs.deserialize_ciphertext(txt);
    if (!(back.c1() == ct.c1()) || !(back.c2() == ct.c2())) ok = false;
    if (!(cs.deserialize_public_key(cs.serialize_public_key(pk)) == pk)) ok = false;
    if (!(cs.deserialize_secret_key(cs.serialize_secret_key(sk)) == sk)) ok = false;
    auto pd = cs.part_decrypt(sk, ct);
    if (!(cs.deserialize_part_decryption_result(cs.serialize_part_decryption_result(pd)) == pd)) ok = false;
    Tensor<CS::PlainText *> pts(2, 3, nullptr);
    pts.flatten();
    const float vals[6] = {0.0f, 1.0f, -1.0f, 255.0f, -65536.0f, 123456.0f};
    for (int i = 0; i < 6; i++) pts.at(i) = new CS::PlainText(cs.make_plaintext(vals[i]));
    pts.reshape({2, 3});
    const std::string bin = cs.serialize_plaintext_tensor(pts);
    auto pb = cs.deserialize_plaintext_tensor(bin);
    if (pb.shape() != pts.shape()) ok = false;
    for (int i = 0; i < 6; i++)
        if (!(*pb[i] == *pts[i])) ok = false;
    if (cs.serialize_plaintext_tensor(pb) != bin) ok = false;
    if (cs.serialize_plaintext(*pts[3]) != "255" || !(cs.deserialize_plaintext("255") == *pts[3])) ok = false;
    {
        CS::CipherText cc = ct;
        Tensor<CS::CipherText *> t(1, &cc);
        std::ofstream("local_bench_fmt_ct.bin", std::ios::binary) << cs.serialize_ciphertext_tensor(t);
    }
    std::ofstream("local_bench_fmt_ct.txt") << txt;
    std::ofstream("local_bench_fmt_pt.bin", std::ios::binary) << bin;
    {
        std::ofstream f("local_bench_fmt_pt.txt");
        for (int i = 0; i < 6; i++) f << cs.serialize_plaintext(*pts[i]) << "\n";
    }
    free_all(pb);
    // ---- the rest of the reference's surface on this path (cpu_cryptosystem.hpp:103-104, 127, 139)
    {
        Mpz bound;
        mpz_setbit(bound.get(), cs.message_bits());
        for (int i = 0; i < 8; i++) {
            auto rp = cs.generate_random_plaintext();
            if (rp.sgn() < 0 || mpz_cmp(rp.get(), bound.get()) >= 0) ok = false;
            auto tr = cs.generate_random_beavers_triplet();
            if (tr.size() != 3 || mpz_cmp_ui(tr[0].get(), 10) >= 0 || mpz_cmp_ui(tr[1].get(), 10) >= 0) ok = false;
            if (!(cs.multiply_plaintexts(tr[0], tr[1]) == tr[2])) ok = false;
        }
        auto again = CS::deserialize(cs.serialize());
        if (again.message_bits() != cs.message_bits() || again.serialize() != cs.serialize()) ok = false;
        // in-place accumulation through the class-group handles, as the node layer writes it
        // (include/smpc/ciphertext_multiplications.hpp:85-98), against add_ciphertexts without re-randomisation
        auto x = cs.encrypt(pk, cs.make_plaintext(5)), y = cs.encrypt(pk, cs.make_plaintext(9));
        cs.set_rerandomize(false);
        auto want = cs.add_ciphertexts(pk, x, y);
        cs.set_rerandomize(true);
        CS::CipherText *res = new CS::CipherText(x);
        auto cl_g = cs.get_hsm2k().Cl_G();
        auto cl_delta = cs.get_hsm2k().Cl_Delta();
        cl_g.nucomp(res->c1(), res->c1(), y.c1());
        cl_delta.nucomp(res->c2(), res->c2(), y.c2());
        if (!(std::as_const(*res).c1() == want.c1()) || !(std::as_const(*res).c2() == want.c2())) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *res)) != 14.0f) ok = false;
        // nucompinv undoes nucomp; nudupl and nupow agree; the principal form is neutral
        QFI back2, sq, p2, neutral;
        cl_g.nucompinv(back2, std::as_const(*res).c1(), y.c1());
        if (!(back2 == x.c1())) ok = false;
        cl_g.nudupl(sq, x.c1());
        cl_g.nupow(p2, x.c1(), Mpz(2ul));
        if (!(sq == p2)) ok = false;
        cl_g.nucomp(neutral, x.c2(), cl_g.one());
        if (!(neutral == x.c2())) ok = false;
        delete res;
        // negate_plaintext_tensor keeps the shape
        Tensor<CS::PlainText *> np = cs.negate_plaintext_tensor(pts);
        if (np.shape() != pts.shape() || cs.get_float_from_plaintext(*np[3]) != -255.0f) ok = false;
        free_all(np);
    }
    free_all(pts);
    // the enum factories
    auto cs2 = make_cryptosystem(SecurityLevel::MEDIUM, 128, Device::GPU);
    auto cs3 = make_cryptosystem(SecurityLevel::MEDIUM, Precision::FP32, 2, Device::GPU);
    if (cs2.message_bits() != 128 || cs3.message_bits() != 128) ok = false;
    std::cout << "  formats: " << (ok ? "ok" : "FAILED") << std::endl;
    if (!ok) throw std::runtime_error("format round trip mismatch");
}

// one HIPCryptoSystem shared by two host threads (the reference's compute server calls one instance from 8 threads,
// include/node/server.hpp:16,185-197): a matrix product (workspace + tables of the context) next to decryptions
// (same workspace, cached table of f), results compared with the single-threaded ones
static void bench_threads(int rounds) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    using CS = decltype(cs);
    auto sk = cs.keygen();
    auto pk = cs.keygen(sk);
    const size_t n = 3, m = 4, p = 4;
    Tensor<CS::PlainText *> pt1(n, m, nullptr), pt2(m, p, nullptr);
    pt1.flatten(); pt2.flatten();
    for (size_t i = 0; i < n * m; i++) pt1.at(i) = new CS::PlainText(cs.make_plaintext(i + 1));
    for (size_t i = 0; i < m * p; i++) pt2.at(i) = new CS::PlainText(cs.make_plaintext((float)(i % 5) - 2.0f));
    pt1.reshape({n, m}); pt2.reshape({m, p});
    auto ct1 = cs.encrypt_tensor(pk, pt1);
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    auto ref = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
    const std::string ref_bytes = cs.serialize_ciphertext_tensor(ref);
    std::atomic<bool> ok{true};
    std::thread ta([&]() {
        for (int r = 0; r < rounds; r++) {
            // alternate shapes so that the workspace is re-sized while the other thread uses the context
            auto res = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
            if (cs.serialize_ciphertext_tensor(res) != ref_bytes) ok = false;
            free_all(res);
        }
    });
    std::thread tb([&]() {
        for (int r = 0; r < rounds; r++) {
            auto dec = cs.decrypt_tensor(sk, ct1);
            dec.flatten();
            for (size_t i = 0; i < n * m; i++) {
                if (cs.get_float_from_plaintext(*dec.at(i)) != (float)(i + 1)) ok = false;
                delete dec.at(i);
            }
        }
    });
    ta.join();
    tb.join();
    // A shared RESULT tensor read by both threads the way the reference reads it -- through the tensor's non-const element
    // pointers, cts.at(i)->c1() (cpu_cryptosystem_tensor_ops.inl:175; the compute server shares tensors between its 8
    // threads): the non-const accessors must not touch the element's block reference (they used to reset it: a race with
    // the other reader and with copies).  Lazy elements, first touched concurrently; every value compared with a
    // single-threaded const read of a second, identical result.
    {
        auto shared = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
        auto check = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
        shared.flatten(); check.flatten();
        const size_t E = n * p;
        std::vector<std::string> want(E);
        for (size_t i = 0; i < E; i++) {
            const CS::CipherText &c = *check.at(i);
            want[i] = c.c1().a().str() + " " + c.c2().b().str();
        }
        auto reader = [&](int start) {
            for (int r = 0; r < rounds; r++)
                for (size_t k = 0; k < E; k++) {
                    const size_t i = (k + start) % E;
                    CS::CipherText *e = shared.at(i);                 // non-const, as a Tensor<CipherText *> hands it out
                    CS::CipherText copy(*e);                          // copies race with the other thread's first read
                    if (e->c1().a().str() + " " + e->c2().b().str() != want[i]) ok = false;
                    if (copy.c1().a().str() + " " + copy.c2().b().str() != want[i]) ok = false;
                }
        };
        std::thread r1(reader, 0), r2(reader, (int)(E / 2));
        r1.join();
        r2.join();
        // a touched element no longer offers its device copy; the values are still what the block holds
        for (size_t i = 0; i < E; i++)
            if (shared.at(i)->block()) ok = false;
        free_all(shared); free_all(check);
    }
    free_all(ref); free_all(ct1); free_all(pt1); free_all(pt2);
    std::cout << "  two threads on one cryptosystem, " << rounds << " rounds each: " << (ok ? "ok" : "FAILED") << std::endl;
    if (!ok) throw std::runtime_error("concurrent use gave a different result");
}

// make_plaintext / get_float_from_plaintext of the product on floats given by their bit patterns (one 8-digit hex word
// per line of `in`): "<decimal plaintext> <bit pattern of the float that comes back>" per line of `out`
static void plaintexts_mode(const char *in, const char *out) {
    auto cs = make_cryptosystem(128, 128, Device::GPU);
    std::ifstream fi(in);
    std::ofstream fo(out);
    std::string tok;
    while (fi >> tok) {
        const uint32_t bits = (uint32_t)std::stoul(tok, nullptr, 16);
        float x;
        memcpy(&x, &bits, 4);
        auto pt = cs.make_plaintext(x);
        const float back = cs.get_float_from_plaintext(pt);
        uint32_t bb;
        memcpy(&bb, &back, 4);
        char buf[16];
        snprintf(buf, sizeof buf, "%08x", bb);
        fo << pt.str() << " " << buf << "\n";
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "Usage: " << argv[0] << " <encrypt_decrypt|ciphertext_matadd|scal_matmul|threshold|ciphertext_matmul|fresh_randomness|affine|beaver_direct|plain_ct_matmul|ciphertext_matmul_matrix|conv2d|conv2d_grouped|sum_pool2d|poly_activation|divide|lookup> [sizes]" << std::endl;
        return 1;
    }
    std::string mode = argv[1];
    try {
        if (mode == "ciphertext_matadd") {
            size_t n = argc > 2 ? std::stoul(argv[2]) : 64, m = argc > 3 ? std::stoul(argv[3]) : 64;
            bench_matadd(n, m);
        } else if (mode == "encrypt_decrypt") {
            size_t n = argc > 2 ? std::stoul(argv[2]) : 64, m = argc > 3 ? std::stoul(argv[3]) : 64;
            bench_encrypt_decrypt(n, m);
        } else if (mode == "scal_matmul") {
            size_t n = argc > 2 ? std::stoul(argv[2]) : 8, m = argc > 3 ? std::stoul(argv[3]) : 64,
                   p = argc > 4 ? std::stoul(argv[4]) : 64;
            const int chain = argc > 5 ? std::stoi(argv[5]) : 50;
            bench_scal_matmul(n, m, p, chain);
        } else if (mode == "ciphertext_matmul") {
            size_t n = argc > 2 ? std::stoul(argv[2]) : 4, m = argc > 3 ? std::stoul(argv[3]) : 4,
                   p = argc > 4 ? std::stoul(argv[4]) : 4, t = argc > 5 ? std::stoul(argv[5]) : 0,
                   parties = argc > 6 ? std::stoul(argv[6]) : 3;
            bench_ciphertext_matmul(n, m, p, t, parties);
        } else if (mode == "plain_ct_matmul") {
            bench_plain_ct_matmul(argc > 2 ? std::stoul(argv[2]) : 3, argc > 3 ? std::stoul(argv[3]) : 5, argc > 4 ? std::stoul(argv[4]) : 4);
        } else if (mode == "conv2d") {
            // B H W C kh kw Co [sh sw ph pw]; by default stride 1 and "same" padding
            auto arg = [&](int i, size_t dflt) { return argc > i ? std::stoul(argv[i]) : dflt; };
            const size_t kh = arg(6, 3), kw = arg(7, 3);
            bench_conv2d(arg(2, 1), arg(3, 6), arg(4, 6), arg(5, 2), kh, kw, arg(8, 2), arg(9, 1), arg(10, 1), arg(11, kh / 2), arg(12, kw / 2));
        } else if (mode == "conv2d_grouped") {
            // B H W C kh kw Co groups [dh dw sh sw ph pw]; by default no dilation, stride 1 and "same" padding
            auto arg = [&](int i, size_t dflt) { return argc > i ? std::stoul(argv[i]) : dflt; };
            const size_t kh = arg(6, 3), kw = arg(7, 3), dh = arg(10, 1), dw = arg(11, 1);
            bench_conv2d_grouped(arg(2, 1), arg(3, 6), arg(4, 6), arg(5, 4), kh, kw, arg(8, 4), arg(9, 4), dh, dw, arg(12, 1), arg(13, 1),
                                 arg(14, (kh - 1) * dh / 2), arg(15, (kw - 1) * dw / 2));
        } else if (mode == "sum_pool2d") {
            // B H W C kh kw [sh sw ph pw]; by default the stride is the window and there is no padding
            auto arg = [&](int i, size_t dflt) { return argc > i ? std::stoul(argv[i]) : dflt; };
            const size_t kh = arg(6, 2), kw = arg(7, 2);
            bench_sum_pool2d(arg(2, 1), arg(3, 6), arg(4, 6), arg(5, 2), kh, kw, arg(8, kh), arg(9, kw), arg(10, 0), arg(11, 0));
        } else if (mode == "ciphertext_matmul_matrix") {
            size_t n = argc > 2 ? std::stoul(argv[2]) : 4, m = argc > 3 ? std::stoul(argv[3]) : 4,
                   p = argc > 4 ? std::stoul(argv[4]) : 4, t = argc > 5 ? std::stoul(argv[5]) : 0,
                   parties = argc > 6 ? std::stoul(argv[6]) : 3;
            bench_ciphertext_matmul_matrix(n, m, p, t, parties);
        } else if (mode == "plaintexts") {
            if (argc < 4) throw std::invalid_argument("plaintexts <in> <out>");
            plaintexts_mode(argv[2], argv[3]);
        } else if (mode == "fresh_randomness") {
            bench_fresh_randomness(argc > 2 ? std::stoul(argv[2]) : 256);
        } else if (mode == "affine") {
            bench_affine(argc > 2 ? std::stoul(argv[2]) : 64);
        } else if (mode == "beaver_direct") {
            bench_beaver_direct(argc > 2 ? std::stoul(argv[2]) : 8);
        } else if (mode == "poly_activation") {
            // elements [runs]: with runs > 0 also the timed comparison with two chained Beaver products
            bench_poly_activation(argc > 2 ? std::stoul(argv[2]) : 64, argc > 3 ? std::stoi(argv[3]) : 0);
        } else if (mode == "divide") {
            // elements [runs]: with runs > 0 also the timed scalar division
            bench_divide(argc > 2 ? std::stoul(argv[2]) : 64, argc > 3 ? std::stoi(argv[3]) : 0);
        } else if (mode == "lookup") {
            // elements [runs]: with runs > 0 also the timed relu
            bench_lookup(argc > 2 ? std::stoul(argv[2]) : 64, argc > 3 ? std::stoi(argv[3]) : 0);
        } else if (mode == "formats") {
            bench_formats();
        } else if (mode == "threads") {
            bench_threads(argc > 2 ? std::stoi(argv[2]) : 4);
        } else if (mode == "threshold") {
            size_t n = argc > 2 ? std::stoul(argv[2]) : 16, m = argc > 3 ? std::stoul(argv[3]) : 16,
                   t = argc > 4 ? std::stoul(argv[4]) : 2, parties = argc > 5 ? std::stoul(argv[5]) : 3;
            bench_threshold(n, m, t, parties);
        } else {
            std::cerr << "Invalid benchmark type" << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
