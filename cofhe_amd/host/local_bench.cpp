// local_bench.cpp -- counterpart of the reference's local harness (benchmarks/local.cpp:65-215,
// benchmarks/benchmark.hpp) on the MI355X engine: same construction of inputs
// (make_plaintext(i+1), encrypt_tensor), same 1+49 chained operations with the per-iteration
// frees, first/last/average/median/total milliseconds per tag.  Additionally reports
// ciphertext-ops/s, the same chain with tensors kept resident in HBM, and writes the serialised
// bytes of the final tensor so a parity checker can compare them.
//
//   ./local_bench <mode> [arguments]
//
// The modes, their arguments and the defaults are the table MODES at the end of this file; ./local_bench without a mode
// prints it.  Every mode is one function over the helpers of the anonymous namespace below: one Fixture (cryptosystem, secret
// key, public key on demand), one clock (ms_since, timed, median_runs), one writer of the files a parity checker reads
// (write_*), tensors that free their elements (plain_tensor, Owned), and the checks and host references the modes share.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <optional>
#include <set>
#include <string>
#include <thread>
#include <utility>

#include "hip_cryptosystem.hpp"
#include "smpc_local.hpp"
#include "spline_table.hpp"

using namespace CoFHE;

namespace {

using CS = HIPCryptoSystem;
using PT = CS::PlainText;
using CT = CS::CipherText;
using Client = LocalSMPCClient<CS>;
using Multiplier = LocalCipherTextMultiplier<CS>;
using Clock = std::chrono::steady_clock;

// ---- fixture: the cryptosystem, a secret key, and the public key once somebody asks for it -------------------------------
struct Fixture {
    CS cs = make_cryptosystem(128, 128, Device::GPU);
    CS::SecretKey sk = cs.keygen();
    // keygen(sk) builds the table of h on first use; a mode that wants it does so up front, a mode that takes the key of its
    // client never calls this
    const CS::PublicKey &pk() {
        if (!pk_) pk_ = cs.keygen(sk);
        return *pk_;
    }

  private:
    std::optional<CS::PublicKey> pk_;
};

std::string client_label(size_t t, size_t parties) {
    return t ? "threshold " + std::to_string(t) + " of " + std::to_string(parties) : std::string("secret key");
}

// t = 0: the client decrypts with the secret key; otherwise by t-of-parties threshold decryption
std::unique_ptr<Client> make_client(Fixture &fx, size_t t, size_t parties) {
    return std::unique_ptr<Client>(t ? new Client(fx.cs, fx.sk, t, parties) : new Client(fx.cs, fx.sk));
}

// fn(client, multiplier, label, threshold) through the secret-key client, then through the 2-of-3 threshold client
template <typename F>
void for_both_clients(Fixture &fx, F fn) {
    for (size_t t : {0, 2}) {
        auto client = make_client(fx, t, 3);
        Multiplier mul(*client);
        fn(*client, mul, client_label(t, 3), t != 0);
    }
}

// ---- clock -----------------------------------------------------------------------------------------------------------------
template <typename TP>
double ms_since(TP t0, TP t1 = TP::clock::now()) {
    return std::chrono::duration<double, std::milli>(t1 - t0).count();
}

// {milliseconds, fn()}: the wall clock of fn and of the device work it enqueued.  Whether the stream is drained before the
// clock starts is the caller's choice (cs.synchronize() in front)
template <typename F>
auto timed(const CS &cs, F fn) {
    const auto t0 = Clock::now();
    auto result = fn();
    cs.synchronize();
    return std::make_pair(ms_since(t0), std::move(result));
}

double median(const std::vector<double> &sorted) { return sorted[sorted.size() / 2]; }

// "<key>": median, "<range_key>": [min, max] of sorted times, for the *_json lines that tools/bench_ops.py reads
struct MsJson {
    const char *key, *range_key;
    const std::vector<double> &sorted;
};
std::ostream &operator<<(std::ostream &o, const MsJson &j) {
    return o << "\"" << j.key << "\": " << median(j.sorted) << ", \"" << j.range_key << "\": [" << j.sorted.front() << ", " << j.sorted.back() << "]";
}

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
            ms.push_back(ms_since(t0, t1));
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

// ---- files for the parity checker --------------------------------------------------------------------------------------------
void write_bytes(const std::string &name, const std::string &bytes) { std::ofstream(name, std::ios::binary) << bytes; }

void write_ciphertexts(const Fixture &fx, const std::string &name, const Tensor<CT *> &t) {
    write_bytes(name, fx.cs.serialize_ciphertext_tensor(t));
}

// one ciphertext as a tensor of one element
void write_ciphertext(const Fixture &fx, const std::string &name, const CT &ct) {
    CT copy = ct;
    write_ciphertexts(fx, name, Tensor<CT *>(1, &copy));
}

void write_absdelta(const Fixture &fx) {
    Mpz ad = fx.cs.discriminant();
    ad.neg();
    write_bytes("local_bench_absdelta.txt", ad.str() + "\n");
}

// ---- tensors -----------------------------------------------------------------------------------------------------------------
template <typename T>
void free_all(const Tensor<T *> &t) {
    for (size_t i = 0; i < t.num_elements(); i++) delete t[i];
}

// A tensor whose elements die with it (0-D tensors included).  Move assignment frees the previous elements first, so
// `res = op(res)` frees each link of a chain as the next one arrives; release() hands the tensor out undeleted.
template <typename T>
class Owned {
  public:
    Owned() = default;
    Owned(Tensor<T *> t) : t_(std::move(t)) {}
    Owned(Owned &&o) noexcept : t_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            free_all(t_);
            t_ = o.release();
        }
        return *this;
    }
    ~Owned() { free_all(t_); }
    Tensor<T *> release() { return std::exchange(t_, Tensor<T *>()); }
    operator const Tensor<T *> &() const { return t_; }
    const Tensor<T *> *operator->() const { return &t_; }
    T *operator[](size_t i) const { return t_[i]; }

  private:
    Tensor<T *> t_;
};

PT plaintext_of(const CS &cs, float v) { return cs.make_plaintext(v); }
PT plaintext_of(const CS &, const Mpz &v) { return v; }

// new plaintexts value_of_index(0), value_of_index(1), ... in this order; floats go through make_plaintext, Mpz as they are
template <typename G>
Owned<PT> plain_tensor(const Fixture &fx, const std::vector<size_t> &shape, G value_of_index) {
    Tensor<PT *> t(shape, nullptr);
    for (size_t i = 0; i < t.num_elements(); i++) t[i] = new PT(plaintext_of(fx.cs, value_of_index(i)));
    return t;
}

float ramp(size_t i) { return (float)(i + 1); }               // the reference's inputs: make_plaintext(i + 1)

template <typename T>
auto from(const std::vector<T> &v) {
    return [&v](size_t i) -> const T & { return v[i]; };
}

// ---- checks ----------------------------------------------------------------------------------------------------------------
bool same_value(const CS &cs, const PT &got, float want) { return cs.get_float_from_plaintext(got) == want; }
bool same_value(const CS &, const PT &got, const Mpz &want) { return got == want; }

// every element of dec is want_of_index(i): a float through get_float_from_plaintext, an Mpz as the residue itself
template <typename W>
bool matches(const CS &cs, const Tensor<PT *> &dec, W want_of_index) {
    bool good = true;
    for (size_t i = 0; i < dec.num_elements(); i++)
        if (!same_value(cs, *dec[i], want_of_index(i))) good = false;
    return good;
}

template <typename W>
bool decrypts_to(const Fixture &fx, const Tensor<CT *> &t, W want_of_index) {
    Owned<PT> dec = fx.cs.decrypt_tensor(fx.sk, t);
    return matches(fx.cs, dec, want_of_index);
}

template <typename V>
bool decrypts_to(const Fixture &fx, const Tensor<CT *> &t, const std::vector<V> &want) {
    return t.num_elements() == want.size() && decrypts_to(fx, t, from(want));
}

std::string c1_text(const CT &c) { return c.c1().a().str() + " " + c.c1().b().str(); }

// all c1 of all these tensors are pairwise distinct
bool distinct_c1(const Vector<Tensor<CT *>> &ts) {
    std::set<std::string> seen;
    size_t total = 0;
    for (const auto &t : ts) {
        total += t.num_elements();
        for (size_t i = 0; i < t.num_elements(); i++) seen.insert(c1_text(*t[i]));
    }
    return seen.size() == total;
}
bool distinct_c1(const Tensor<CT *> &t) { return distinct_c1(Vector<Tensor<CT *>>{t}); }

// (n x m) . (m x p) of a_of_index and b_of_index over row-major flat indices.  Like the convolution below: small integers,
// exact in float in any order
template <typename A, typename B>
std::vector<float> matmul_reference(size_t n, size_t m, size_t p, A a_of_index, B b_of_index) {
    std::vector<float> out(n * p);
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < p; k++) {
            float want = 0;
            for (size_t j = 0; j < m; j++) want += a_of_index(i * m + j) * b_of_index(j * p + k);
            out[i * p + k] = want;
        }
    return out;
}

// image B x H x W x C (channels last), filters kh x kw x C/groups x Co, output column co reads the channels of group
// co / (Co / groups).  groups = 1 and dh = dw = 1 is the plain convolution; groups = Co = C with weights 1 is sum pooling
struct ConvGeometry {
    size_t B, H, W, C, kh, kw, Co, groups, dh, dw, sh, sw, ph, pw;
};

// term(o, xi, wi) for every product of the convolution: output o gains image element xi times filter element wi (flat indices)
template <typename Term>
void conv_terms(const ConvGeometry &g, size_t Ho, size_t Wo, Term term) {
    const size_t Cg = g.C / g.groups, Cog = g.Co / g.groups;
    for (size_t bb = 0; bb < g.B; bb++)
        for (size_t oy = 0; oy < Ho; oy++)
            for (size_t ox = 0; ox < Wo; ox++)
                for (size_t co = 0; co < g.Co; co++)
                    for (size_t dy = 0; dy < g.kh; dy++)
                        for (size_t dx = 0; dx < g.kw; dx++) {
                            const size_t y = oy * g.sh + dy * g.dh, xx = ox * g.sw + dx * g.dw;
                            if (y < g.ph || y - g.ph >= g.H || xx < g.pw || xx - g.pw >= g.W) continue;
                            for (size_t ci = 0; ci < Cg; ci++)
                                term(((bb * Ho + oy) * Wo + ox) * g.Co + co, ((bb * g.H + (y - g.ph)) * g.W + (xx - g.pw)) * g.C + (co / Cog) * Cg + ci,
                                     ((dy * g.kw + dx) * Cg + ci) * g.Co + co);
                        }
}

// the B x Ho x Wo x Co outputs of xval and wval over flat indices
template <typename X, typename Wt>
std::vector<float> conv_reference(const ConvGeometry &g, size_t Ho, size_t Wo, X xval, Wt wval) {
    std::vector<float> out(g.B * Ho * Wo * g.Co);
    conv_terms(g, Ho, Wo, [&](size_t o, size_t xi, size_t wi) { out[o] += xval(xi) * wval(wi); });
    return out;
}

// the same for plaintexts, exactly, mod 2^k
std::vector<Mpz> conv_reference_mod(const ConvGeometry &g, size_t Ho, size_t Wo, const Tensor<PT *> &x, const Tensor<PT *> &w, uint32_t k) {
    std::vector<Mpz> out(g.B * Ho * Wo * g.Co);
    conv_terms(g, Ho, Wo, [&](size_t o, size_t xi, size_t wi) { mpz_addmul(out[o].get(), x[xi]->get(), w[wi]->get()); });
    for (auto &v : out) mpz_fdiv_r_2exp(v.get(), v.get(), k);
    return out;
}

float conv_xval(size_t i) { return (float)(i % 11) - 4.0f; }
float conv_wval(size_t i) { return (float)(i % 7) - 3.0f; }      // weights of both signs, zeros among them

// ---- arguments ---------------------------------------------------------------------------------------------------------------
struct Args {
    int argc;
    char **argv;
    size_t operator()(int i, size_t dflt) const { return argc > i ? std::stoul(argv[i]) : dflt; }
    int integer(int i, int dflt) const { return argc > i ? std::stoi(argv[i]) : dflt; }
};

// a warm-up pass and `runs` timed passes of fn (a ciphertext tensor, freed after its pass), each from a drained stream; the
// times come back sorted.  before() runs in front of every pass, outside its clock.
template <typename F, typename P>
std::vector<double> median_runs(const CS &cs, int runs, F fn, P before) {
    std::vector<double> ms;
    for (int pass = 0; pass <= runs; pass++) {
        before();
        cs.synchronize();
        auto run = timed(cs, [&]() -> Owned<CT> { return fn(); });
        if (pass) ms.push_back(run.first);
    }
    std::sort(ms.begin(), ms.end());
    return ms;
}
template <typename F>
std::vector<double> median_runs(const CS &cs, int runs, F fn) {
    return median_runs(cs, runs, fn, []() {});
}

struct ConvResult {
    bool ok;
    size_t Ho, Wo;
};

// The three image modes: encrypt the image conv_xval, run op(pk, image) once under the tag, decrypt and compare with
// conv_reference (inside the run, as ever); the output must be B x . x . x Co
template <typename Op, typename Wt>
ConvResult conv_check(Fixture &fx, const std::string &tag, const ConvGeometry &g, Wt wval, Op op) {
    auto &cs = fx.cs;
    const auto &pk = fx.pk();
    Owned<PT> x = plain_tensor(fx, {g.B, g.H, g.W, g.C}, conv_xval);
    Owned<CT> cx = cs.encrypt_tensor(pk, x);
    Benchmark b(tag);
    bool ok = true;
    std::vector<size_t> oshape;
    b.run([&]() {
        Owned<CT> res = op(pk, cx);
        oshape = res->shape();
        if (!decrypts_to(fx, res, conv_reference(g, oshape[1], oshape[2], conv_xval, wval))) ok = false;
    }, 1);
    b.print_summary();
    const bool four = oshape.size() == 4;
    return {ok && four && oshape[0] == g.B && oshape[3] == g.Co, four ? oshape[1] : 0, four ? oshape[2] : 0};
}

}  // namespace

static void bench_matadd(const Args &arg) {
    const size_t n = arg(2, 64), m = arg(3, 64);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &pk = fx.pk();
    Owned<PT> pt1 = plain_tensor(fx, {n, m}, ramp), pt2 = plain_tensor(fx, {n, m}, ramp);
    Owned<CT> ct1 = cs.encrypt_tensor(pk, pt1);
    Owned<CT> ct2 = cs.encrypt_tensor(pk, pt2);
    Benchmark b("ciphertext_matadd (API: Tensor<CipherText*> in and out each op)");
    std::string final_bytes;
    double api_chain_ms = 0, api_ser_ms = 0;
    b.run([&]() {
        auto chain = timed(cs, [&]() {
            Owned<CT> res = cs.add_ciphertext_tensors(pk, ct1, ct2);
            for (int i = 0; i < 49; ++i) res = cs.add_ciphertext_tensors(pk, res, ct2);
            return res;
        });
        const auto t1 = Clock::now();
        final_bytes = cs.serialize_ciphertext_tensor(chain.second);
        chain.second = Owned<CT>();
        api_chain_ms = chain.first;
        api_ser_ms = ms_since(t1);
    }, 1);
    std::cout << "  of which 50 API calls " << api_chain_ms << " ms, serialising the result " << api_ser_ms << " ms" << std::endl;
    b.print_summary();
    std::cout << "  " << 50.0 * n * m / (b.ms[0] * 1e-3) << " ciphertext-ops/s (host marshalling included)" << std::endl;
    Benchmark r("ciphertext_matadd (tensors resident in HBM)");
    std::string resident_bytes;
    r.run([&]() {
        auto d1 = cs.upload(ct1);
        auto d2 = cs.upload(ct2);
        auto chain = timed(cs, [&]() {
            auto res = cs.add_ciphertext_tensors(d1, d2);
            for (int i = 0; i < 49; ++i) res = cs.add_ciphertext_tensors(res, d2);
            return res;
        });
        const double ms = chain.first;
        std::cout << "  resident chain of 50: " << ms << " ms, " << 50.0 * n * m / (ms * 1e-3) << " ciphertext-ops/s" << std::endl;
        Owned<CT> back = cs.download(chain.second);
        resident_bytes = cs.serialize_ciphertext_tensor(back);
    }, 1);
    r.print_summary();
    std::cout << "  API chain and resident chain agree: " << (final_bytes == resident_bytes ? "yes" : "NO") << std::endl;
    write_ciphertexts(fx, "local_bench_matadd_ct1.bin", ct1);
    write_ciphertexts(fx, "local_bench_matadd_ct2.bin", ct2);
    write_bytes("local_bench_matadd_out.bin", final_bytes);
    write_absdelta(fx);
    std::cout << "n: " << n << " m: " << m << std::endl;
}

static void bench_scal_matmul(const Args &arg) {
    const size_t n = arg(2, 8), m = arg(3, 64), p = arg(4, 64);
    int chain = arg.integer(5, 50);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &pk = fx.pk();
    Owned<PT> pt1 = plain_tensor(fx, {n, m}, ramp), pt2 = plain_tensor(fx, {m, p}, ramp);
    Owned<CT> ct1 = cs.encrypt_tensor(pk, pt1);
    // the reference draws a fresh Enc(0) inside every product (tensor_ops.inl:352); a fixed one makes the run
    // reproducible for the parity checker
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    if (m != p) chain = 1;                                   // the chain re-feeds the n x p result as the n x m operand
    Benchmark b("scal_matmul (1 + " + std::to_string(chain - 1) + " chained products, benchmarks/local.cpp:177-197)");
    std::string final_bytes;
    b.run([&]() {
        Owned<CT> res = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
        for (int i = 0; i < chain - 1; ++i) res = cs.scal_ciphertext_tensors(pk, pt2, res, &zero);
        final_bytes = cs.serialize_ciphertext_tensor(res);
    }, 1);
    b.print_summary();
    std::cout << "  " << (double)chain * n * p / (b.ms[0] * 1e-3) << " output ciphertexts/s" << std::endl;
    write_bytes("local_bench_scal_s.bin", cs.serialize_plaintext_tensor(pt2));
    write_ciphertexts(fx, "local_bench_scal_cts.bin", ct1);
    write_ciphertext(fx, "local_bench_scal_zero.bin", zero);
    write_bytes("local_bench_scal_out.bin", final_bytes);
    write_absdelta(fx);
    std::cout << "n: " << n << " m: " << m << " p: " << p << " chain: " << chain << std::endl;
}

// counterpart of benchmark_encrypt_decrypt (benchmarks/local.cpp:22-63), with the check the
// reference omits: every plaintext must come back
static void bench_encrypt_decrypt(const Args &arg) {
    const size_t n = arg(2, 64), m = arg(3, 64);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const auto &pk = fx.pk();
    Owned<PT> pts = plain_tensor(fx, {n, m}, ramp);
    Benchmark b("encrypt_decrypt");
    bool ok = true;
    double enc_first_ms = 0, enc_again_ms = 0, dec_ms = 0;
    b.run([&]() {
        // whole encrypt_tensor calls, h^r and pk^r included: the first builds the fixed-base tables of h and pk
        // (one chain of ~1000 squarings each), later calls find them in the context
        auto first = timed(cs, [&]() -> Owned<CT> { return cs.encrypt_tensor(pk, pts); });
        auto again = timed(cs, [&]() -> Owned<CT> { return cs.encrypt_tensor(pk, pts); });
        const auto t2 = Clock::now();
        first.second = Owned<CT>();
        Owned<PT> res = cs.decrypt_tensor(sk, again.second);
        dec_ms = ms_since(t2);
        enc_first_ms = first.first;
        enc_again_ms = again.first;
        if (!matches(cs, res, ramp)) ok = false;
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
        Tensor<CT *> ta(&a), tb(&bb);
        Tensor<PT *> ts(&three);
        Owned<CT> sum = cs.add_ciphertext_tensors(pk, ta, tb);
        Owned<CT> tri = cs.scal_ciphertext_tensors(pk, ts, ta);
        if (!sum->is_zero_degree() || !tri->is_zero_degree()) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *sum->get_value())) != 12.0f) ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *tri->get_value())) != 21.0f) ok = false;
        // a second call gives a different ciphertext of the same value (fresh r)
        Owned<CT> sum2 = cs.add_ciphertext_tensors(pk, ta, tb);
        if (sum2->get_value()->c1() == sum->get_value()->c1()) ok = false;
        // ... and deterministic when asked, so that a checker can compare bytes
        cs.set_rerandomize(false);
        Owned<CT> dsum = cs.add_ciphertext_tensors(pk, ta, tb);
        Owned<CT> dtri = cs.scal_ciphertext_tensors(pk, ts, ta);
        write_ciphertext(fx, "local_bench_scalar_a.bin", a);
        write_ciphertext(fx, "local_bench_scalar_b.bin", bb);
        write_ciphertext(fx, "local_bench_scalar_sum.bin", *dsum->get_value());
        write_ciphertext(fx, "local_bench_scalar_tri.bin", *dtri->get_value());
        cs.set_rerandomize(true);
        write_absdelta(fx);
    }
    b.print_summary();
    std::cout << "  encrypt_tensor (h^r, pk^r included): first call " << enc_first_ms << " ms (builds the tables of h and pk), next call "
              << enc_again_ms << " ms = " << n * m / (enc_again_ms * 1e-3) << " ciphertexts/s; decrypt_tensor " << dec_ms << " ms" << std::endl;
    std::cout << "  roundtrip and homomorphic checks: " << (ok ? "ok" : "FAILED") << std::endl;
    std::cout << "n: " << n << " m: " << m << std::endl;
    if (!ok) throw std::runtime_error("decryption mismatch");
}

// fresh randomness per element (TensorRandomness::PerElement): encrypt_tensor gives every ciphertext its own r, the tensor
// operations re-randomise their outputs, rerandomize_ciphertext_tensor does it on request; everything decrypts as before
static void bench_fresh_randomness(const Args &arg) {
    const size_t n = arg(2, 256);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &pk = fx.pk();
    std::vector<float> want(n);
    for (size_t i = 0; i < n; i++) want[i] = (float)((long)i - (long)(n / 2));
    Owned<PT> pts = plain_tensor(fx, {n}, from(want));
    auto times = [&](float factor) { return [&want, factor](size_t i) { return factor * want[i]; }; };
    bool ok = true;
    Owned<CT> shared = cs.encrypt_tensor(pk, pts);            // default mode: one r for the tensor
    cs.synchronize();
    for (size_t i = 1; i < n; i++)
        if (c1_text(*shared[i]) != c1_text(*shared[0])) ok = false;
    cs.set_tensor_randomness(TensorRandomness::PerElement);
    auto [enc_ms, ct] = timed(cs, [&]() -> Owned<CT> { return cs.encrypt_tensor(pk, pts); });
    const bool enc_distinct = distinct_c1(ct), enc_dec = decrypts_to(fx, ct, times(1.0f));
    Owned<CT> sum = cs.add_ciphertext_tensors(pk, ct, ct);
    CS::PlainText p3 = cs.make_plaintext(3);
    Tensor<PT *> three(n, &p3);
    Owned<CT> tri = cs.scal_ciphertext_tensors(pk, three, ct);
    Owned<CT> neg = cs.negate_ciphertext_tensor(pk, ct);
    auto [rr_ms, rr] = timed(cs, [&]() -> Owned<CT> { return cs.rerandomize_ciphertext_tensor(pk, shared); });
    const bool ops_distinct = distinct_c1(sum) && distinct_c1(tri) && distinct_c1(neg) && distinct_c1(rr);
    const bool ops_dec = decrypts_to(fx, sum, times(2.0f)) && decrypts_to(fx, tri, times(3.0f)) && decrypts_to(fx, neg, times(-1.0f)) &&
                         decrypts_to(fx, rr, times(1.0f));
    ok = ok && enc_distinct && enc_dec && ops_distinct && ops_dec;
    write_ciphertexts(fx, "local_bench_fresh_ct.bin", ct);
    write_ciphertexts(fx, "local_bench_fresh_rerand.bin", rr);
    write_absdelta(fx);
    std::cout << "  per-element encrypt_tensor: " << enc_ms << " ms, rerandomize_ciphertext_tensor: " << rr_ms << " ms (" << n
              << " ciphertexts)" << std::endl;
    std::cout << "  distinct c1: encrypt " << (enc_distinct ? "yes" : "NO") << ", add / scal / negate / rerandomize "
              << (ops_distinct ? "yes" : "NO") << "; decryption: encrypt " << (enc_dec ? "yes" : "NO") << ", ops " << (ops_dec ? "yes" : "NO")
              << std::endl;
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("fresh randomness check failed");
}

// differences and plaintext addends (sub_ciphertext_tensors, invert_ciphertext_tensor, add / sub_plaintext_tensor,
// plaintext_sub_ciphertext_tensor) against decryption, in the default mode, per element, 0-D and in PerElement mode
static void bench_affine(const Args &arg) {
    const size_t n = arg(2, 64);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const auto &pk = fx.pk();
    std::vector<float> a(n), b(n), m(n);
    for (size_t i = 0; i < n; i++) {
        a[i] = (float)((long)(i * 7 % 101) - 50);
        b[i] = (float)((long)(i * 13 % 89) - 44);
        m[i] = (float)((long)(i * 5 % 61) - 30);
    }
    Owned<PT> pa = plain_tensor(fx, {n}, from(a)), pb = plain_tensor(fx, {n}, from(b)), pm = plain_tensor(fx, {n}, from(m));
    auto a_minus_b = [&](size_t i) { return a[i] - b[i]; };
    auto a_plus_m = [&](size_t i) { return a[i] + m[i]; };
    auto m_minus_a = [&](size_t i) { return m[i] - a[i]; };
    Owned<CT> ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
    cs.synchronize();
    bool ok = true;
    auto [sub_ms, diff] = timed(cs, [&]() -> Owned<CT> { return cs.sub_ciphertext_tensors(pk, ca, cb); });
    auto [neg_add_ms, diff_ref] = timed(cs, [&]() -> Owned<CT> {
        Owned<CT> nb = cs.negate_ciphertext_tensor(pk, cb);
        return cs.add_ciphertext_tensors(pk, ca, nb);
    });
    auto [plain_ms, sum_m] = timed(cs, [&]() -> Owned<CT> { return cs.add_plaintext_tensor(pk, ca, pm); });
    auto [enc_add_ms, sum_ref] = timed(cs, [&]() -> Owned<CT> {
        Owned<CT> em = cs.encrypt_tensor(pk, pm);
        return cs.add_ciphertext_tensors(pk, ca, em);
    });
    Owned<CT> dif_m = cs.sub_plaintext_tensor(pk, ca, pm);
    Owned<CT> m_dif = cs.plaintext_sub_ciphertext_tensor(pk, pm, ca);
    Owned<CT> inv = cs.invert_ciphertext_tensor(ca);
    const bool dec_ok = decrypts_to(fx, diff, a_minus_b) && decrypts_to(fx, diff_ref, a_minus_b) && decrypts_to(fx, sum_m, a_plus_m) &&
                        decrypts_to(fx, sum_ref, a_plus_m) && decrypts_to(fx, dif_m, [&](size_t i) { return a[i] - m[i]; }) &&
                        decrypts_to(fx, m_dif, m_minus_a) && decrypts_to(fx, inv, [&](size_t i) { return -a[i]; });
    // the plaintext addend leaves c1 alone: a tensor that shared its c1 still does
    bool c1_kept = true;
    for (size_t i = 0; i < n; i++)
        if (c1_text(*sum_m[i]) != c1_text(*ca[0]) || c1_text(*dif_m[i]) != c1_text(*ca[0])) c1_kept = false;
    // shape errors and the 0-D forms
    bool shape_ok = false;
    try {
        Tensor<CT *> shorter(n > 1 ? n - 1 : 2, ca[0]);
        (void)cs.sub_ciphertext_tensors(pk, ca, shorter);
    } catch (const std::invalid_argument &e) {
        shape_ok = std::string(e.what()) == "Tensor shapes must be equal";
    }
    bool scalar_ok = true;
    {
        CT x = *ca[1 % n], y = *cb[1 % n];
        PT mm = *pm[1 % n];
        Tensor<CT *> tx(&x), ty(&y);
        Tensor<PT *> tm(&mm);
        Owned<CT> d0 = cs.sub_ciphertext_tensors(pk, tx, ty);
        Owned<CT> s0 = cs.add_plaintext_tensor(pk, tx, tm);
        Owned<CT> i0 = cs.invert_ciphertext_tensor(tx);
        if (!d0->is_zero_degree() || !s0->is_zero_degree() || !i0->is_zero_degree()) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *d0->get_value())) != a[1 % n] - b[1 % n]) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *s0->get_value())) != a[1 % n] + m[1 % n]) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, *i0->get_value())) != -a[1 % n]) scalar_ok = false;
        // the scalar difference is re-randomised like the scalar sum: a second call gives another ciphertext
        auto d1 = cs.sub_ciphertexts(pk, x, y);
        if (d1.c1() == d0->get_value()->c1()) scalar_ok = false;
        if (cs.get_float_from_plaintext(cs.decrypt(sk, d1)) != a[1 % n] - b[1 % n]) scalar_ok = false;
    }
    write_ciphertexts(fx, "local_bench_affine_sub.bin", diff);
    write_ciphertexts(fx, "local_bench_affine_plain.bin", m_dif);
    // PerElement mode: the same results with a fresh r per element
    cs.set_tensor_randomness(TensorRandomness::PerElement);
    Owned<CT> fdiff = cs.sub_ciphertext_tensors(pk, ca, cb);
    Owned<CT> fsum = cs.add_plaintext_tensor(pk, ca, pm);
    Owned<CT> fmdif = cs.plaintext_sub_ciphertext_tensor(pk, pm, ca);
    const bool fresh_ok = (n < 2 || (distinct_c1(fdiff) && distinct_c1(fsum) && distinct_c1(fmdif))) && decrypts_to(fx, fdiff, a_minus_b) &&
                          decrypts_to(fx, fsum, a_plus_m) && decrypts_to(fx, fmdif, m_minus_a);
    cs.set_tensor_randomness(TensorRandomness::None);
    ok = dec_ok && c1_kept && shape_ok && scalar_ok && fresh_ok;
    write_absdelta(fx);
    std::cout << "  sub_ciphertext_tensors " << sub_ms << " ms, negate + add " << neg_add_ms << " ms; add_plaintext_tensor " << plain_ms
              << " ms, encrypt_tensor + add " << enc_add_ms << " ms (" << n << " ciphertexts, host wall clock, first calls)" << std::endl;
    std::cout << "  decryption: " << (dec_ok ? "yes" : "NO") << ", c1 kept by the plaintext addend: " << (c1_kept ? "yes" : "NO")
              << ", shape error: " << (shape_ok ? "yes" : "NO") << ", 0-D forms: " << (scalar_ok ? "yes" : "NO") << ", per-element mode: "
              << (fresh_ok ? "yes" : "NO") << std::endl;
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("affine check failed");
}

// the Beaver element product with LocalCipherTextMultiplier::set_direct_differences: x*y mod 2^k as without it
static void bench_beaver_direct(const Args &arg) {
    const size_t n = arg(2, 8);
    Fixture fx;
    auto &cs = fx.cs;
    Client client(cs, fx.sk);
    Multiplier mul(client);
    const auto &pk = client.network_public_key();
    auto xval = [](size_t i) { return (float)((long)(i % 7) - 3); };
    auto yval = [](size_t i) { return (float)((long)(i % 5) + 1); };
    Owned<PT> px = plain_tensor(fx, {n}, xval), py = plain_tensor(fx, {n}, yval);
    Owned<CT> cx = cs.encrypt_tensor(pk, px), cy = cs.encrypt_tensor(pk, py);
    bool ok = true;
    double ms[2] = {0, 0};
    for (int pass = 0; pass < 2; pass++)          // a warm-up pass builds the tables; the second is timed
        for (int direct = 0; direct < 2; direct++) {
            mul.set_direct_differences(direct != 0);
            cs.synchronize();
            auto run = timed(cs, [&]() -> Owned<CT> { return mul.multiply_ciphertext_tensors(cx, cy); });
            ms[direct] = run.first;
            if (!decrypts_to(fx, run.second, [&](size_t i) { return xval(i) * yval(i); })) ok = false;
            if (direct && pass) write_ciphertexts(fx, "local_bench_beaver_direct.bin", run.second);
        }
    write_absdelta(fx);
    std::cout << "  " << n << " element products: reference sequence " << ms[0] << " ms, direct differences " << ms[1]
              << " ms (host wall clock, triplet generation and decryptions included)" << std::endl;
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("beaver product mismatch");
}

// a polynomial activation on a ciphertext tensor from one opened value per element
// (LocalCipherTextMultiplier::evaluate_polynomial_ciphertext_tensor), through the single-key and the 2-of-3 threshold client:
// degree 3 with a negative coefficient over n elements, checked against p(x) mod 2^k from GMP on the host; prints
// client.decrypted_elements(), which must equal the element count.  runs > 0: also the timed comparison with two chained
// Beaver products
static void bench_poly_activation(const Args &arg) {
    const size_t n = arg(2, 64);
    const int runs = arg.integer(3, 0);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const uint32_t k = cs.message_bits();
    Mpz c[4] = {Mpz(5ul), Mpz(3ul), Mpz(7ul), Mpz(11ul)};
    c[1].neg();
    mpz_fdiv_r_2exp(c[1].get(), c[1].get(), k);                 // -3 mod 2^k
    Tensor<PT *> coef(4, nullptr);
    for (size_t j = 0; j < 4; j++) coef[j] = &c[j];
    std::vector<Mpz> want(n);
    Owned<PT> px = plain_tensor(fx, {n}, [&](size_t i) {
        // 0, 1, 2^k - 1, 2^(k-1), small values of both signs, then uniform ones
        Mpz x = i < 2 ? Mpz((unsigned long)i) : i < 8 ? cs.make_plaintext((float)((long)i - 5)) : cs.random_plaintext(k);
        if (i == 2 || i == 3) mpz_ui_pow_ui(x.get(), 2, i == 2 ? k : k - 1);
        if (i == 2) mpz_sub_ui(x.get(), x.get(), 1);
        for (int j = 3; j >= 0; j--) {                          // Horner mod 2^k
            mpz_mul(want[i].get(), want[i].get(), x.get());
            mpz_add(want[i].get(), want[i].get(), c[j].get());
            mpz_fdiv_r_2exp(want[i].get(), want[i].get(), k);
        }
        return x;
    });
    bool ok = true;
    for_both_clients(fx, [&](Client &client, Multiplier &mul, const std::string &who, bool threshold) {
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        cs.synchronize();
        auto [ms, res] = timed(cs, [&]() -> Owned<CT> { return mul.evaluate_polynomial_ciphertext_tensor(coef, cx); });
        const bool pass = decrypts_to(fx, res, want) && client.decrypted_elements() == n;
        if (!threshold) write_ciphertexts(fx, "local_bench_poly_activation.bin", res);
        std::cout << "  " << who << ": degree 3 over " << n << " elements, decrypted_elements " << client.decrypted_elements() << ", " << ms
                  << " ms (host wall clock, tuple generation and the decryption included): " << (pass ? "ok" : "FAILED") << std::endl;
        ok = ok && pass;
        if (threshold) return;
        // the parts on their own: the square of the tensor and of one 0-D element, the Taylor shift (q_0 = p(x)), and the
        // two-base power product [x]^2 o [x]^3 = [5 x]
        const auto &pk = client.network_public_key();
        Owned<CT> sq = mul.square_ciphertext_tensor(cx);
        Owned<CT> sq0 = mul.square_ciphertext_tensor(Tensor<CT *>(cx[1 % n]));
        Owned<PT> dsq = cs.decrypt_tensor(sk, sq);
        auto dsq0 = cs.decrypt(sk, *sq0->get_value());
        auto q = cs.poly_shift_plaintext_tensor(coef, px);
        Mpz two(2ul), three(3ul);
        Vector<Tensor<PT *>> exps{Tensor<PT *>(n, &two), Tensor<PT *>(n, &three)};
        Vector<Tensor<CT *>> bases{cx, cx};
        Owned<CT> dot = cs.pow_dot_ciphertext_tensors(pk, exps, bases);
        Owned<PT> ddot = cs.decrypt_tensor(sk, dot);
        bool parts = q.size() == 4 && sq0->is_zero_degree();
        for (size_t i = 0; i < n; i++) {
            Mpz x2, x5;
            mpz_mul(x2.get(), px[i]->get(), px[i]->get());
            mpz_fdiv_r_2exp(x2.get(), x2.get(), k);
            mpz_mul_ui(x5.get(), px[i]->get(), 5);
            mpz_fdiv_r_2exp(x5.get(), x5.get(), k);
            if (!(*dsq[i] == x2) || !(*ddot[i] == x5) || !(*q[0].at(i) == want[i])) parts = false;
            if (i == 1 % n && !(dsq0 == x2)) parts = false;
        }
        std::cout << "  square (1-D and 0-D), poly_shift_plaintext_tensor, pow_dot_ciphertext_tensors: " << (parts ? "ok" : "FAILED") << std::endl;
        ok = ok && parts;
        for (auto &t : q) free_all(t);
    });
    write_absdelta(fx);
    if (runs > 0) {
        // x^3 twice on the same input, single-key client: the polynomial (0, 0, 0, 1) with one opened value per element, and
        // (x * x) * x by two chained Beaver products with direct differences (four opened values per element, two rounds);
        // alternating, `runs` timed calls each after a warm-up of both; medians and extremes on one line for tools/bench_ops.py
        Client client(cs, sk);
        Multiplier mul(client);
        mul.set_direct_differences(true);
        Mpz zero(0ul), one(1ul);
        Tensor<PT *> cube(4, &zero);
        cube[3] = &one;
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        std::vector<Mpz> cubed(n);
        for (size_t i = 0; i < n; i++) {
            mpz_pow_ui(cubed[i].get(), px[i]->get(), 3);
            mpz_fdiv_r_2exp(cubed[i].get(), cubed[i].get(), k);
        }
        std::vector<double> ms[2];
        size_t opened[2] = {0, 0};
        bool same = true;
        for (int pass = 0; pass <= runs; pass++)
            for (int chained = 0; chained < 2; chained++) {
                const size_t before = client.decrypted_elements();
                cs.synchronize();
                auto run = timed(cs, [&]() -> Owned<CT> {
                    if (!chained) return mul.evaluate_polynomial_ciphertext_tensor(cube, cx);
                    Owned<CT> sq = mul.multiply_ciphertext_tensors(cx, cx);
                    return mul.multiply_ciphertext_tensors(sq, cx);
                });
                if (pass) ms[chained].push_back(run.first);
                opened[chained] = client.decrypted_elements() - before;
                if (!decrypts_to(fx, run.second, cubed)) same = false;
            }
        for (auto &v : ms) std::sort(v.begin(), v.end());
        std::cout << "compare_json: {\"E\": " << n << ", \"degree\": 3, \"runs\": " << runs << ", " << MsJson{"poly_ms", "poly_ms_min_max", ms[0]} << ", "
                  << MsJson{"chained_products_ms", "chained_ms_min_max", ms[1]} << ", \"chained_over_poly\": " << median(ms[1]) / median(ms[0])
                  << ", \"opened_poly\": " << opened[0] << ", \"opened_chained\": " << opened[1] << ", \"agree\": " << (same ? "true" : "false") << "}"
                  << std::endl;
        ok = ok && same;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("polynomial activation mismatch");
}

// division of a ciphertext tensor by public divisors from one opened value per element
// (LocalCipherTextMultiplier::divide_ciphertext_tensor_by_plaintext), through the single-key and the 2-of-3 threshold client:
// a scalar divisor, a per-channel divisor (4 channels) and truncate by 2^16 over n elements with |x| < 2^40 of both signs (a
// wrap then has probability below 2^-80 per element at k = 128); every decrypted element must be floor(x / D) from GMP on the
// host or one less; prints client.decrypted_elements() per call, which must equal the element count.  runs > 0: the median
// wall clock of `runs` scalar divisions on one line for tools/bench_ops.py
static void bench_divide(const Args &arg) {
    const size_t n = arg(2, 64);
    const int runs = arg.integer(3, 0);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const uint32_t k = cs.message_bits();
    const size_t C = n % 4 == 0 ? 4 : 1;
    std::vector<Mpz> xs(n);                                         // signed values
    Owned<PT> px = plain_tensor(fx, {n}, [&](size_t i) {
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
        return m;
    });
    Mpz seven(7ul), per_channel[4] = {Mpz(3ul), Mpz(1000003ul), Mpz(1ul), Mpz(2ul)};
    mpz_mul_2exp(per_channel[1].get(), per_channel[1].get(), 20);   // beyond one limb
    Tensor<PT *> dscalar(1, &seven), dchan(C, nullptr);
    for (size_t c = 0; c < C; c++) dchan[c] = &per_channel[c];
    const uint32_t t_bits = 16;
    // got is floor(x / d) or one less, as residues mod 2^k
    auto floor_or_one_less = [&](const Mpz &got, const Mpz &x, const Mpz &d) {
        Mpz q, a, b;
        mpz_fdiv_q(q.get(), x.get(), d.get());
        mpz_fdiv_r_2exp(a.get(), q.get(), k);
        mpz_sub_ui(q.get(), q.get(), 1);
        mpz_fdiv_r_2exp(b.get(), q.get(), k);
        return got == a || got == b;
    };
    bool ok = true;
    for_both_clients(fx, [&](Client &client, Multiplier &mul, const std::string &who, bool threshold) {
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        Mpz two_t;
        mpz_setbit(two_t.get(), t_bits);
        Tensor<PT *> dtrunc(1, &two_t);
        const char *names[3] = {"scalar divisor 7", "per-channel divisors", "truncate by 2^16"};
        for (int what = 0; what < 3; what++) {
            const Tensor<PT *> &div = what == 0 ? dscalar : what == 1 ? dchan : dtrunc;
            const size_t before = client.decrypted_elements();
            cs.synchronize();
            auto [ms, res] = timed(cs, [&]() -> Owned<CT> {
                return what == 2 ? mul.truncate_ciphertext_tensor(cx, t_bits) : mul.divide_ciphertext_tensor_by_plaintext(cx, div);
            });
            const size_t opened = client.decrypted_elements() - before;
            Owned<PT> dec = cs.decrypt_tensor(sk, res);
            bool pass = opened == n;
            for (size_t i = 0; i < n; i++)
                if (!floor_or_one_less(*dec->at(i), xs[i], *div[i % div.num_elements()])) pass = false;
            if (!threshold && what == 0) write_ciphertexts(fx, "local_bench_divide.bin", res);
            std::cout << "  " << who << ": " << names[what] << " over " << n << " elements, opened_values " << opened << ", " << ms
                      << " ms (host wall clock, pair generation and the decryption included): " << (pass ? "ok" : "FAILED") << std::endl;
            ok = ok && pass;
        }
        if (threshold) return;
        // the parts on their own: one 0-D element, the plaintext division, an invalid divisor, and the mean of 2 x 2 windows
        Owned<CT> q0 = mul.divide_ciphertext_tensor_by_plaintext(Tensor<CT *>(cx[2 % n]), Tensor<PT *>(&seven));
        auto dq0 = cs.decrypt(sk, *q0->get_value());
        Owned<PT> pq = cs.divide_plaintext_tensor(px, dscalar);
        bool parts = q0->is_zero_degree() && floor_or_one_less(dq0, xs[2 % n], seven);
        for (size_t i = 0; i < n; i++) {
            Mpz q, a;
            mpz_fdiv_q(q.get(), xs[i].get(), seven.get());
            mpz_fdiv_r_2exp(a.get(), q.get(), k);
            if (!(*pq->at(i) == a)) parts = false;
        }
        Mpz zero(0ul);
        bool refused = false;
        try {
            (void)mul.divide_ciphertext_tensor_by_plaintext(cx, Tensor<PT *>(1, &zero));
        } catch (const std::invalid_argument &) {
            refused = true;
        }
        parts = parts && refused;
        if (n % 4 == 0) {
            Tensor<CT *> img = cx;
            img.reshape({1, 2, 2, n / 4});
            Owned<CT> avg = mul.avg_pool2d_ciphertext_tensor(img, {2, 2}, {2, 2});
            Owned<PT> davg = cs.decrypt_tensor(sk, avg);
            const Mpz four(4ul);
            for (size_t c = 0; c < n / 4; c++) {
                Mpz s;
                for (size_t p = 0; p < 4; p++) mpz_add(s.get(), s.get(), xs[p * (n / 4) + c].get());
                if (!floor_or_one_less(*davg[c], s, four)) parts = false;
            }
        }
        std::cout << "  0-D division, divide_plaintext_tensor, the refusal of divisor 0, avg_pool2d: " << (parts ? "ok" : "FAILED") << std::endl;
        ok = ok && parts;
    });
    write_absdelta(fx);
    if (runs > 0) {
        Client client(cs, sk);
        Multiplier mul(client);
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        const auto ms = median_runs(cs, runs, [&]() { return mul.divide_ciphertext_tensor_by_plaintext(cx, dscalar); });
        std::cout << "divide_json: {\"E\": " << n << ", \"runs\": " << runs << ", " << MsJson{"divide_ms", "divide_ms_min_max", ms} << "}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("division mismatch");
}

// exact division of a ciphertext tensor by small public divisors from one opened value per element and round
// (LocalCipherTextMultiplier::divide_exact_ciphertext_tensor_by_plaintext and what is built on it), through the single-key and
// the 2-of-3 threshold client: a scalar divisor, per-channel divisors (4 channels), Nearest rounding, truncate_exact by 2^8 (one
// round) and by 2^16 (two rounds), the remainder, the decomposition of 20-bit values into 3 digits of 8 bits and the exact 2 x 2
// average pool, over n elements with |x| < 2^40 of both signs (a wrap then has probability below 2^-80 per element and round at
// k = 128); every decrypted element must EQUAL the plaintext integer from GMP on the host; prints client.decrypted_elements() per
// call, which must equal the element count times the rounds.  runs > 0: the checks through the single-key client only, then the
// median wall clock of `runs` scalar divisions on one line for tools/bench_ops.py
static void bench_divide_exact(const Args &arg) {
    const size_t n = arg(2, 64);
    const int runs = arg.integer(3, 0);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const uint32_t k = cs.message_bits();
    const size_t C = n % 4 == 0 ? 4 : 1;
    std::vector<Mpz> xs(n), smalls(n);                              // signed values: up to 40 bits, and up to 20 bits
    auto residue = [&](const Mpz &x) {
        Mpz m;
        mpz_fdiv_r_2exp(m.get(), x.get(), k);
        return m;
    };
    auto draw = [&](size_t i, uint32_t bits) {
        // 0, 1, -1, the ends of the range, then uniform ones of both signs
        Mpz x = i < 2 ? Mpz((unsigned long)i) : cs.random_plaintext(bits);
        if (i == 3 || i == 4) {
            mpz_set_ui(x.get(), 0);
            mpz_setbit(x.get(), bits);
            mpz_sub_ui(x.get(), x.get(), 1);
        }
        if (i == 2) mpz_set_ui(x.get(), 1);
        if (i == 2 || i == 4 || (i > 4 && i % 2)) x.neg();
        return x;
    };
    Owned<PT> px = plain_tensor(fx, {n}, [&](size_t i) { return residue(xs[i] = draw(i, 40)); });
    Owned<PT> psmall = plain_tensor(fx, {n}, [&](size_t i) { return residue(smalls[i] = draw(i, 19)); });
    Mpz seven(7ul), per_channel[4] = {Mpz(3ul), Mpz(100ul), Mpz(1ul), Mpz(8ul)}, two8(256ul), two16(65536ul);
    Tensor<PT *> dscalar(1, &seven), dchan(C, nullptr);
    for (size_t c = 0; c < C; c++) dchan[c] = &per_channel[c];
    // floor(x / d), or the nearest integer with ties up, as a residue mod 2^k
    auto quotient = [&](const Mpz &x, const Mpz &d, bool nearest) {
        Mpz q, h;
        mpz_fdiv_q_2exp(h.get(), d.get(), 1);
        if (nearest) mpz_add(h.get(), h.get(), x.get());
        mpz_fdiv_q(q.get(), nearest ? h.get() : x.get(), d.get());
        return residue(q);
    };
    bool ok = true;
    for_both_clients(fx, [&](Client &client, Multiplier &mul, const std::string &who, bool threshold) {
        if (threshold && runs > 0) return;                          // the timed leg checks through the single-key client only
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        const char *names[6] = {"scalar divisor 7", "per-channel divisors", "nearest by 7", "truncate_exact by 2^8", "truncate_exact by 2^16",
                                "remainder by 7"};
        for (int what = 0; what < 6; what++) {
            const Tensor<PT *> &div = what == 1 ? dchan : dscalar;
            const size_t rounds = what == 4 ? 2 : 1, before = client.decrypted_elements();
            cs.synchronize();
            auto [ms, res] = timed(cs, [&]() -> Owned<CT> {
                switch (what) {
                case 2: return mul.divide_exact_ciphertext_tensor_by_plaintext(cx, div, Multiplier::Rounding::Nearest);
                case 3: return mul.truncate_exact_ciphertext_tensor(cx, 8);
                case 4: return mul.truncate_exact_ciphertext_tensor(cx, 16);
                case 5: return mul.remainder_ciphertext_tensor(cx, div);
                default: return mul.divide_exact_ciphertext_tensor_by_plaintext(cx, div);
                }
            });
            const size_t opened = client.decrypted_elements() - before;
            Owned<PT> dec = cs.decrypt_tensor(sk, res);
            bool pass = opened == n * rounds;
            for (size_t i = 0; i < n; i++) {
                Mpz want;
                if (what == 5)
                    mpz_fdiv_r(want.get(), xs[i].get(), seven.get());
                else
                    want = quotient(xs[i], what == 3 ? two8 : what == 4 ? two16 : *div[i % div.num_elements()], what == 2);
                if (!(*dec->at(i) == want)) pass = false;
            }
            if (!threshold && what == 0) write_ciphertexts(fx, "local_bench_divide_exact.bin", res);
            std::cout << "  " << who << ": " << names[what] << " over " << n << " elements, opened_values " << opened << ", " << ms
                      << " ms (host wall clock, tuple generation and the decryption included): " << (pass ? "ok" : "FAILED") << std::endl;
            ok = ok && pass;
        }
        // 3 digits of 8 bits of 20-bit values: two digits in [0, 256) and the signed top part, recombined
        {
            Owned<CT> cs20 = cs.encrypt_tensor(client.network_public_key(), psmall);
            const size_t before = client.decrypted_elements();
            auto digits = mul.decompose_ciphertext_tensor(cs20, 8, 3);
            const size_t opened = client.decrypted_elements() - before;
            bool pass = opened == 2 * n && digits.size() == 3;
            std::vector<Owned<PT>> dec;
            for (auto &d : digits) {
                Owned<CT> own(d);
                dec.emplace_back(cs.decrypt_tensor(sk, own));
            }
            for (size_t i = 0; pass && i < n; i++) {
                Mpz d0, d1, top, sum;
                mpz_fdiv_r_2exp(d0.get(), smalls[i].get(), 8);
                mpz_fdiv_q_2exp(top.get(), smalls[i].get(), 8);
                mpz_fdiv_r_2exp(d1.get(), top.get(), 8);
                mpz_fdiv_q_2exp(top.get(), top.get(), 8);
                if (!(*dec[0]->at(i) == d0) || !(*dec[1]->at(i) == d1) || !(*dec[2]->at(i) == residue(top))) pass = false;
                mpz_mul_2exp(sum.get(), top.get(), 8);
                mpz_add(sum.get(), sum.get(), d1.get());
                mpz_mul_2exp(sum.get(), sum.get(), 8);
                mpz_add(sum.get(), sum.get(), d0.get());
                if (!(sum == smalls[i])) pass = false;
            }
            std::cout << "  " << who << ": decompose into 3 digits of 8 bits over " << n << " elements, opened_values " << opened << ": "
                      << (pass ? "ok" : "FAILED") << std::endl;
            ok = ok && pass;
        }
        if (threshold) return;
        // the parts on their own: one 0-D element, the plaintext quotients and remainders, the rows, the refusals of the divisors 0
        // and 4097, and the exact mean of 2 x 2 windows
        Owned<CT> q0 = mul.divide_exact_ciphertext_tensor_by_plaintext(Tensor<CT *>(cx[2 % n]), Tensor<PT *>(&seven));
        auto dq0 = cs.decrypt(sk, *q0->get_value());
        bool parts = q0->is_zero_degree() && dq0 == quotient(xs[2 % n], seven, false);
        auto qm = cs.divmod_plaintext_tensor(px, dscalar);
        Owned<PT> pq(qm[0]), pm(qm[1]);
        Owned<PT> rows = cs.divx_rows_plaintext_tensor(px, dscalar);
        for (size_t i = 0; i < n; i++) {
            Mpz m;
            mpz_fdiv_r(m.get(), xs[i].get(), seven.get());
            if (!(*pq->at(i) == quotient(xs[i], seven, false)) || !(*pm->at(i) == m)) parts = false;
            for (unsigned long j = 0; j < 7; j++) {
                Mpz t = quotient(xs[i], seven, false);
                if (mpz_get_ui(m.get()) + j >= 7) {
                    mpz_add_ui(t.get(), t.get(), 1);
                    t = residue(t);
                }
                if (!(*rows->at(i * 7 + j) == t)) parts = false;
            }
        }
        Mpz zero(0ul), big(4097ul);
        for (Mpz *bad : {&zero, &big}) {
            bool refused = false;
            try {
                (void)mul.divide_exact_ciphertext_tensor_by_plaintext(cx, Tensor<PT *>(1, bad));
            } catch (const std::invalid_argument &) {
                refused = true;
            }
            parts = parts && refused;
        }
        if (n % 4 == 0) {
            Tensor<CT *> img = cx;
            img.reshape({1, 2, 2, n / 4});
            Owned<CT> avg = mul.avg_pool2d_exact_ciphertext_tensor(img, {2, 2}, {2, 2});
            Owned<PT> davg = cs.decrypt_tensor(sk, avg);
            const Mpz four(4ul);
            for (size_t c = 0; c < n / 4; c++) {
                Mpz s;
                for (size_t p = 0; p < 4; p++) mpz_add(s.get(), s.get(), xs[p * (n / 4) + c].get());
                if (!(*davg[c] == quotient(s, four, false))) parts = false;
            }
        }
        std::cout << "  0-D division, divmod_plaintext_tensor, divx_rows_plaintext_tensor, the refusals of the divisors 0 and 4097, avg_pool2d_exact: "
                  << (parts ? "ok" : "FAILED") << std::endl;
        ok = ok && parts;
    });
    write_absdelta(fx);
    if (runs > 0) {
        Client client(cs, sk);
        Multiplier mul(client);
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        const auto ms = median_runs(cs, runs, [&]() { return mul.divide_exact_ciphertext_tensor_by_plaintext(cx, dscalar); });
        std::cout << "divide_exact_json: {\"E\": " << n << ", \"runs\": " << runs << ", "
                  << MsJson{"divide_exact_ms", "divide_exact_ms_min_max", ms} << "}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("exact division mismatch");
}

// table lookups on a ciphertext tensor from one opened value per element (LocalCipherTextMultiplier::lookup_ciphertext_tensor),
// through the single-key and the 2-of-3 threshold client: a random 8-bit table, relu and max at 8 bits over n elements of the
// whole signed 8-bit range, and a 2 x 2 max pool of them (n a multiple of 4); every decrypted element must EQUAL the plaintext
// computation; prints the opened values per call (n for a lookup, 3 per output for the 2 x 2 pool) and whether all c1 of one
// tuple tensor are pairwise distinct in the default randomness mode.  runs > 0: the median wall clock of `runs` relu calls on
// one line for tools/bench_ops.py
static void bench_lookup(const Args &arg) {
    const size_t n = arg(2, 64);
    const int runs = arg.integer(3, 0);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
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
    Owned<PT> px = plain_tensor(fx, {n}, [&](size_t i) { return residue(xs[i]); });
    Owned<PT> py = plain_tensor(fx, {n}, [&](size_t i) { return residue(ys[i]); });
    std::vector<Mpz> g((size_t)1 << bits);                          // any public function: 256 uniform k-bit plaintexts
    Tensor<PT *> table(g.size(), nullptr);
    for (size_t j = 0; j < g.size(); j++) {
        g[j] = cs.random_plaintext(k);
        table[j] = &g[j];
    }
    auto g_of = [&](long x) -> const Mpz & { return g[(size_t)(x & ((1L << bits) - 1))]; };
    bool ok = true;
    for_both_clients(fx, [&](Client &client, Multiplier &mul, const std::string &who, bool threshold) {
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px), cy = cs.encrypt_tensor(client.network_public_key(), py);
        const char *names[3] = {"random 8-bit table", "relu at 8 bits", "max at 8 bits"};
        for (int what = 0; what < 3; what++) {
            std::vector<Mpz> want(n);
            for (size_t i = 0; i < n; i++) want[i] = what == 0 ? g_of(xs[i]) : residue(what == 1 ? std::max(xs[i], 0L) : std::max(xs[i], ys[i]));
            const size_t before = client.decrypted_elements();
            cs.synchronize();
            auto [ms, res] = timed(cs, [&]() -> Owned<CT> {
                return what == 0 ? mul.lookup_ciphertext_tensor(table, cx) : what == 1 ? mul.relu_ciphertext_tensor(cx, bits)
                                                                                       : mul.max_ciphertext_tensors(cx, cy, bits);
            });
            const size_t opened = client.decrypted_elements() - before;
            const bool pass = decrypts_to(fx, res, want) && opened == n;
            if (!threshold && what == 1) write_ciphertexts(fx, "local_bench_lookup.bin", res);
            std::cout << "  " << who << ": " << names[what] << " over " << n << " elements, opened_values " << opened << ", " << ms
                      << " ms (host wall clock, tuple generation and the decryption included): " << (pass ? "ok" : "FAILED") << std::endl;
            ok = ok && pass;
        }
        if (n % 4 == 0) {
            Tensor<CT *> img = cx;
            img.reshape({1, 2, 2, n / 4});
            const size_t before = client.decrypted_elements();
            Owned<CT> pooled = mul.max_pool2d_ciphertext_tensor(img, {2, 2}, {2, 2}, bits);
            const size_t opened = client.decrypted_elements() - before;
            std::vector<Mpz> want(n / 4);
            for (size_t c = 0; c < n / 4; c++) {
                long m = xs[c];
                for (size_t p = 1; p < 4; p++) m = std::max(m, xs[p * (n / 4) + c]);
                want[c] = residue(m);
            }
            const bool pass = decrypts_to(fx, pooled, want) && opened == 3 * (n / 4);
            std::cout << "  " << who << ": 2 x 2 max pool, opened_values " << opened << " for " << n / 4 << " outputs, two rounds: " << (pass ? "ok" : "FAILED")
                      << std::endl;
            ok = ok && pass;
        }
        if (threshold) return;
        // the parts on their own: one 0-D element, the plaintext rows, the refusals, and the randomness of a tuple tensor
        Owned<CT> y0 = mul.lookup_ciphertext_tensor(table, Tensor<CT *>(cx[1 % n]));
        bool parts = y0->is_zero_degree() && cs.decrypt(sk, *y0->get_value()) == g_of(xs[1 % n]);
        Mpz three(3ul);
        Owned<PT> rows = cs.lut_rotate_plaintext_tensor(table, Tensor<PT *>(1, &three));
        for (size_t j = 0; j < g.size(); j++) parts = parts && *rows[j] == g[(j + 3) % g.size()];
        int refused = 0;
        try {
            (void)mul.lookup_ciphertext_tensor(Tensor<PT *>(3, &three), cx);       // 3 entries: no power of two
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
        auto tuples = client.get_lookup_tuples(4, table);
        size_t count = 0;
        for (auto &t : tuples) count += t.num_elements();
        const bool distinct = default_mode && count == 4 + 4 * g.size() && distinct_c1(tuples);
        std::cout << "  " << 4 + 4 * g.size() << " ciphertexts of the tuples of 4 elements, default randomness mode, distinct c1: "
                  << (distinct ? "yes" : "NO") << std::endl;
        ok = ok && distinct;
        for (auto &t : tuples) free_all(t);
    });
    write_absdelta(fx);
    if (runs > 0) {
        Client client(cs, sk);
        Multiplier mul(client);
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        const auto ms = median_runs(cs, runs, [&]() { return mul.relu_ciphertext_tensor(cx, bits); });
        std::cout << "lookup_json: {\"E\": " << n << ", \"bits\": " << bits << ", \"runs\": " << runs << ", " << MsJson{"relu_ms", "relu_ms_min_max", ms}
                  << "}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("lookup mismatch");
}

// the exact sign, ReLU and max of values on a window of `bits` bits from digit comparisons
// (LocalCipherTextMultiplier::is_nonnegative_ciphertext_tensor, relu_wide_ciphertext_tensor, max_wide_ciphertext_tensors),
// through the single-key and the 2-of-3 threshold client: the edges -2^(bits-1), -1, 0, 1, 2^(bits-1) - 1, then uniform values of
// the window (the max runs on their halves, whose difference stays in it).  Every decrypted element must EQUAL the integer
// computation; prints the opened values per element (3 for the sign, 5 for ReLU and max) and whether all c1 of one tuple tensor
// are pairwise distinct in the default randomness mode.  runs > 0: medians of `runs` calls of the wide ReLU, of its tuple
// generation, its opening and its closing step, and of the 8-bit lookup ReLU over the same element count, on one line
static void bench_compare(const Args &arg) {
    const size_t n = arg(2, 256);
    const uint32_t bits = (uint32_t)arg(3, 32), digit_bits = (uint32_t)arg(4, 0);
    const int runs = arg.integer(5, 0);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const uint32_t k = cs.message_bits();
    if (bits < 3 || bits > 64 || bits > k) throw std::invalid_argument("compare: a window of 3 to min(k, 64) bits");
    const uint32_t d = digit_bits ? digit_bits : cs.cmp_pick_digit_bits(bits);
    const auto shape = cs.cmp_shape(bits, d);
    auto window = [&](uint64_t u) { return bits == 64 ? (int64_t)u : (int64_t)(u << (64 - bits)) >> (64 - bits); };      // sign-extended
    const int64_t lo = window((uint64_t)1 << (bits - 1)), hi = (int64_t)(((uint64_t)1 << (bits - 1)) - 1);
    std::vector<int64_t> xs(n), ys(n);
    const int64_t fixed[5] = {lo, -1, 0, 1, hi};
    for (size_t i = 0; i < n; i++) {
        xs[i] = i < 5 ? fixed[i] : window(mpz_get_ui(cs.random_plaintext(bits).get()));
        ys[i] = i < 5 ? fixed[4 - i] : window(mpz_get_ui(cs.random_plaintext(bits).get()));
    }
    auto residue = [&](int64_t v) {                                 // v mod 2^k
        Mpz m;
        mpz_set_si(m.get(), (long)v);
        mpz_fdiv_r_2exp(m.get(), m.get(), k);
        return m;
    };
    Owned<PT> px = plain_tensor(fx, {n}, [&](size_t i) { return residue(xs[i]); });
    Owned<PT> pa = plain_tensor(fx, {n}, [&](size_t i) { return residue(xs[i] >> 1); });
    Owned<PT> pb = plain_tensor(fx, {n}, [&](size_t i) { return residue(ys[i] >> 1); });
    std::cout << "compare: " << n << " elements, window " << bits << " bits, " << shape.digits << " digits of " << d << " bits, " << shape.entries
              << " + " << ((size_t)4 << shape.digits) << " ciphertexts of tuples per element" << std::endl;
    bool ok = true;
    for_both_clients(fx, [&](Client &client, Multiplier &mul, const std::string &who, bool threshold) {
        const auto &pk = client.network_public_key();
        Owned<CT> cx = cs.encrypt_tensor(pk, px), ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
        const char *names[3] = {"sign", "relu", "max"};
        const size_t per_element[3] = {3, 5, 5};
        for (int what = 0; what < 3; what++) {
            std::vector<Mpz> want(n);
            for (size_t i = 0; i < n; i++)
                want[i] = residue(what == 0 ? (xs[i] >= 0 ? 1 : 0) : what == 1 ? std::max<int64_t>(xs[i], 0) : std::max(xs[i] >> 1, ys[i] >> 1));
            const size_t before = client.decrypted_elements();
            cs.synchronize();
            auto [ms, res] = timed(cs, [&]() -> Owned<CT> {
                return what == 0 ? mul.is_nonnegative_ciphertext_tensor(cx, bits, digit_bits)
                                 : what == 1 ? mul.relu_wide_ciphertext_tensor(cx, bits, digit_bits) : mul.max_wide_ciphertext_tensors(ca, cb, bits - 1, digit_bits);
            });
            const size_t opened = client.decrypted_elements() - before;
            const bool pass = decrypts_to(fx, res, want) && opened == per_element[what] * n;
            if (!threshold && what == 1) write_ciphertexts(fx, "local_bench_compare.bin", res);
            std::cout << "  " << who << ": " << names[what] << " over " << n << " elements, opened_values_per_element " << (double)opened / (double)n << ", "
                      << ms << " ms (host wall clock, tuple generation and the decryptions included): " << (pass ? "ok" : "FAILED") << std::endl;
            ok = ok && pass;
        }
        if (threshold) return;
        // the parts on their own: one 0-D element, the plaintext rows, the refusals, and the randomness of a tuple tensor
        Owned<CT> y0 = mul.relu_wide_ciphertext_tensor(Tensor<CT *>(cx[4 % n]), bits, digit_bits);
        bool parts = y0->is_zero_degree() && cs.decrypt(sk, *y0->get_value()) == residue(std::max<int64_t>(xs[4 % n], 0));
        Mpz five(5ul);
        Owned<PT> rows = cs.cmp_rows_plaintext_tensor(Tensor<PT *>(1, &five), bits, d);
        for (uint32_t j = 0; j < shape.digits; j++)
            for (uint32_t c = 0; c < (1u << d); c++) {
                const int64_t rj = (int64_t)((5u >> (j * d < 32 ? j * d : 31)) & ((1u << d) - 1u)), s = rj > (int64_t)c ? 1 : rj < (int64_t)c ? -1 : 0;
                parts = parts && mpz_cmp_si(rows[(j << d) + c]->get(), (long)(s * ((int64_t)1 << j))) == 0;
            }
        int refused = 0;
        try {
            (void)mul.is_nonnegative_ciphertext_tensor(cx, 65);
        } catch (const std::invalid_argument &) {
            refused++;
        }
        try {
            (void)mul.is_nonnegative_ciphertext_tensor(cx, 64, 5);                  // 13 digits: the closing lookup would have 14 bits
        } catch (const std::invalid_argument &) {
            refused++;
        }
        try {
            (void)mul.max_wide_ciphertext_tensors(ca, cb, 64);
        } catch (const std::invalid_argument &) {
            refused++;
        }
        parts = parts && refused == 3;
        std::cout << "  0-D relu, cmp_rows_plaintext_tensor, the refusals of 65 bits, of 13 digits and of a max at 64 bits: " << (parts ? "ok" : "FAILED")
                  << std::endl;
        ok = ok && parts;
        const bool default_mode = cs.tensor_randomness() == TensorRandomness::None;
        auto tuples = client.get_comparison_tuples(4, bits, d);
        size_t count = 0;
        for (auto &t : tuples) count += t.num_elements();
        const bool distinct = default_mode && count == 4 + 4 * (size_t)shape.entries && distinct_c1(tuples);
        std::cout << "  " << count << " ciphertexts of the tuples of 4 elements, default randomness mode, distinct c1: " << (distinct ? "yes" : "NO")
                  << std::endl;
        ok = ok && distinct;
        for (auto &t : tuples) free_all(t);
    });
    write_absdelta(fx);
    if (runs > 0) {
        Client client(cs, sk);
        Multiplier mul(client);
        const auto &pk = client.network_public_key();
        Owned<CT> cx = cs.encrypt_tensor(pk, px);
        Owned<PT> p8 = plain_tensor(fx, {n}, [&](size_t i) { return residue((int64_t)(int8_t)(xs[i] & 0xFF)); });
        Owned<CT> c8 = cs.encrypt_tensor(pk, p8);
        const auto relu_ms = median_runs(cs, runs, [&]() { return mul.relu_wide_ciphertext_tensor(cx, bits, digit_bits); });
        const auto sign_ms = median_runs(cs, runs, [&]() { return mul.is_nonnegative_ciphertext_tensor(cx, bits, digit_bits); });
        const auto relu8_ms = median_runs(cs, runs, [&]() { return mul.relu_ciphertext_tensor(c8, 8); });
        // the three parts of round 1 on their own: the tuples, the opening of x - r, the closing compositions
        std::vector<double> tuples_ms, open_ms, close_ms;
        for (int pass = 0; pass <= runs; pass++) {
            cs.synchronize();
            auto a = timed(cs, [&]() { return client.get_comparison_tuples(n, bits, d); });
            Owned<CT> diff = cs.sub_ciphertext_tensors(pk, cx, a.second[0]);
            cs.synchronize();
            auto b = timed(cs, [&]() -> Owned<PT> { return client.decrypt_tensor(diff); });
            cs.synchronize();
            auto c = timed(cs, [&]() { return cs.cmp_close_ciphertext_tensor(b.second, a.second[1], bits, d); });
            free_all(c.second.pairs);
            free_all(c.second.wrap);
            for (auto &t : a.second) free_all(t);
            if (pass) {
                tuples_ms.push_back(a.first);
                open_ms.push_back(b.first);
                close_ms.push_back(c.first);
            }
        }
        for (auto *v : {&tuples_ms, &open_ms, &close_ms}) std::sort(v->begin(), v->end());
        std::cout << "compare_json: {\"E\": " << n << ", \"bits\": " << bits << ", \"digit_bits\": " << d << ", \"digits\": " << shape.digits
                  << ", \"runs\": " << runs << ", " << MsJson{"relu_wide_ms", "relu_wide_ms_min_max", relu_ms} << ", "
                  << MsJson{"sign_ms", "sign_ms_min_max", sign_ms} << ", " << MsJson{"tuples_ms", "tuples_ms_min_max", tuples_ms} << ", "
                  << MsJson{"open_ms", "open_ms_min_max", open_ms} << ", " << MsJson{"close_ms", "close_ms_min_max", close_ms} << ", "
                  << MsJson{"relu_lookup_8bit_ms", "relu_lookup_8bit_ms_min_max", relu8_ms} << "}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("compare mismatch");
}

// a piecewise-polynomial activation on a ciphertext tensor from one opened value per element
// (LocalCipherTextMultiplier::evaluate_spline_ciphertext_tensor), through the single-key and the 2-of-3 threshold client: the
// logistic sigmoid on [-8, 8) as 2^bits pieces of degree d over a (shift + bits)-bit window, 40 fraction bits out
// (make_spline_table), over n elements outside the lowest segment.  Every decrypted element must EQUAL the table's own value on
// the element's piece or on the piece below, and lie within the builder's reported error of the sigmoid; prints the opened
// values per call, the worst error, and whether all c1 of one tuple tensor are pairwise distinct in the default randomness mode.
// runs > 0: the median wall clock of tuple generation, opening (difference and decryption) and closing on one line for
// tools/bench_ops.py
static void bench_spline(const Args &arg) {
    const size_t n = arg(2, 256);
    const int runs = arg.integer(3, 0);
    const uint32_t bits = (uint32_t)arg(4, 5), shift = (uint32_t)arg(5, 11), d = (uint32_t)arg(6, 2);
    if (shift + bits < 4 || shift + bits > 40) throw std::invalid_argument("spline: a window of 4 to 40 bits");
    const uint32_t in_frac = shift + bits - 4, out_frac = 40;          // the window is [-8, 8)
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const uint32_t k = cs.message_bits();
    auto sigmoid = [](double v) { return 1.0 / (1.0 + std::exp(-v)); };
    const SplineTable st = make_spline_table(sigmoid, bits, shift, d, in_frac, out_frac);
    Owned<PT> table = st.tensor<PT>();
    const long half = 1L << (bits - 1), seg = 1L << shift;
    const long lo = -(half - 1) * seg, hi = half * seg;                // everything but the lowest segment
    // the ends of the range, 0, -1, 1, both sides of a segment boundary, then uniform ones
    std::vector<long> xs(n);
    const long fixed[8] = {lo, hi - 1, 0, -1, 1, seg - 1, seg, -seg};
    for (size_t i = 0; i < n; i++)
        xs[i] = i < 8 ? std::min(std::max(fixed[i], lo), hi - 1) : lo + (long)(mpz_get_ui(cs.random_plaintext(62).get()) % (unsigned long)(hi - lo));
    auto residue = [&](long v) {                                    // v mod 2^k
        Mpz m((unsigned long)(v < 0 ? -v : v));
        if (v < 0) m.neg();
        mpz_fdiv_r_2exp(m.get(), m.get(), k);
        return m;
    };
    auto sigma_of = [&](long x) { return x >= 0 ? x / seg : -((-x + seg - 1) / seg); };
    auto piece_of = [&](long sigma) { return (uint32_t)(sigma & ((1L << bits) - 1)); };
    auto piece_value = [&](long x, long sigma) {                    // S_p(x) mod 2^k for the piece p of origin sigma 2^shift
        Mpz acc;
        for (uint32_t i = d + 1; i-- > 0;) {
            const int64_t c = st.coef[(size_t)piece_of(sigma) * (d + 1) + i];
            mpz_mul_si(acc.get(), acc.get(), x - sigma * seg);
            if (c < 0) mpz_sub_ui(acc.get(), acc.get(), (unsigned long)(0 - (uint64_t)c));
            else mpz_add_ui(acc.get(), acc.get(), (unsigned long)c);
        }
        mpz_fdiv_r_2exp(acc.get(), acc.get(), k);
        return acc;
    };
    Owned<PT> px = plain_tensor(fx, {n}, [&](size_t i) { return residue(xs[i]); });
    bool ok = true;
    double worst = 0;
    // every element is its own piece's value or the value of the piece below, and that value is close to the sigmoid
    auto check = [&](const Tensor<CT *> &res) {
        Owned<PT> dec = cs.decrypt_tensor(sk, res);
        bool good = dec->num_elements() == n;
        for (size_t i = 0; good && i < n; i++) {
            const long so = sigma_of(xs[i]);
            const bool own = *dec[i] == piece_value(xs[i], so), below = shift != 0 && *dec[i] == piece_value(xs[i], so - 1);
            good = own || below;
            const long su = own ? so : so - 1;
            const double err = (double)std::fabs(st.value(piece_of(su), (long double)(xs[i] - su * seg)) -
                                                 (long double)sigmoid((double)std::ldexp((long double)xs[i], -(int)in_frac)));
            worst = std::max(worst, err);
        }
        return good;
    };
    for_both_clients(fx, [&](Client &client, Multiplier &mul, const std::string &who, bool threshold) {
        Owned<CT> cx = cs.encrypt_tensor(client.network_public_key(), px);
        const size_t before = client.decrypted_elements();
        cs.synchronize();
        auto [ms, res] = timed(cs, [&]() -> Owned<CT> { return mul.evaluate_spline_ciphertext_tensor(table, cx, bits, shift); });
        const size_t opened = client.decrypted_elements() - before;
        const bool pass = check(res) && opened == n;
        if (!threshold) write_ciphertexts(fx, "local_bench_spline.bin", res);
        std::cout << "  " << who << ": sigmoid, " << ((size_t)1 << bits) << " pieces of degree " << d << " over a " << shift + bits << "-bit window, " << n
                  << " elements, opened_values " << opened << ", " << ms << " ms (host wall clock, tuple generation and the decryption included): "
                  << (pass ? "ok" : "FAILED") << std::endl;
        ok = ok && pass;
        if (threshold) return;
        // the parts on their own: one 0-D element, the plaintext rows, the refusals, and the randomness of a tuple tensor
        Owned<CT> y0 = mul.evaluate_spline_ciphertext_tensor(table, Tensor<CT *>(cx[1 % n]), bits, shift);
        const long s1 = sigma_of(xs[1 % n]);
        const Mpz v0 = cs.decrypt(sk, *y0->get_value());
        bool parts = y0->is_zero_degree() && (v0 == piece_value(xs[1 % n], s1) || v0 == piece_value(xs[1 % n], s1 - 1));
        // row 0 of the mask r = 0 is piece 0 shifted by nothing: the table's own coefficients mod 2^k
        Mpz zero;
        Owned<PT> rows = cs.spline_rows_plaintext_tensor(table, Tensor<PT *>(1, &zero), bits, shift);
        parts = parts && rows->num_elements() == ((size_t)(d + 1) << bits);
        for (uint32_t i = 0; parts && i <= d; i++) {
            Mpz c = *table[i];
            mpz_fdiv_r_2exp(c.get(), c.get(), k);
            parts = *rows[i] == c;
        }
        int refused = 0;
        try {
            (void)mul.evaluate_spline_ciphertext_tensor(table, cx, bits + 1, shift);       // the table has 2^bits pieces
        } catch (const std::invalid_argument &) {
            refused++;
        }
        try {
            (void)mul.evaluate_spline_ciphertext_tensor(table, cx, bits, k - bits + 1);    // the window leaves k
        } catch (const std::invalid_argument &) {
            refused++;
        }
        parts = parts && refused == 2 && client.decrypted_elements() == before + n + 1;     // refused before anything was drawn
        std::cout << "  0-D spline, spline_rows_plaintext_tensor, the refusals of a wrong piece count and of a window beyond k: " << (parts ? "ok" : "FAILED")
                  << std::endl;
        ok = ok && parts;
        const bool default_mode = cs.tensor_randomness() == TensorRandomness::None;
        auto tuples = client.get_spline_tuples(4, table, bits, shift);
        size_t count = 0;
        for (auto &t : tuples) count += t.num_elements();
        const size_t want_count = 4 + 4 * ((size_t)(d + 1) << bits);
        const bool distinct = default_mode && count == want_count && distinct_c1(tuples);
        std::cout << "  " << want_count << " ciphertexts of the tuples of 4 elements, default randomness mode, distinct c1: " << (distinct ? "yes" : "NO")
                  << std::endl;
        ok = ok && distinct;
        for (auto &t : tuples) free_all(t);
    });
    ok = ok && worst <= st.max_error;
    std::cout << "spline_error: worst " << worst << " reported " << st.max_error << std::endl;
    write_absdelta(fx);
    if (runs > 0) {
        Client client(cs, sk);
        const auto &pk = client.network_public_key();
        Owned<CT> cx = cs.encrypt_tensor(pk, px);
        std::vector<double> t_tuples, t_open, t_close;
        for (int pass = 0; pass <= runs; pass++) {                  // a warm-up pass, then the timed ones, each from a drained stream
            cs.synchronize();
            auto a = timed(cs, [&]() { return client.get_spline_tuples(n, table, bits, shift); });
            auto b = timed(cs, [&]() -> Owned<PT> {
                Owned<CT> diff = cs.sub_ciphertext_tensors(pk, cx, a.second[0]);
                return client.decrypt_tensor(diff);
            });
            auto c = timed(cs, [&]() -> Owned<CT> { return cs.spline_close_ciphertext_tensor(b.second, a.second[1], bits, shift); });
            for (auto &t : a.second) free_all(t);
            if (pass) t_tuples.push_back(a.first), t_open.push_back(b.first), t_close.push_back(c.first);
        }
        for (auto *v : {&t_tuples, &t_open, &t_close}) std::sort(v->begin(), v->end());
        std::cout << "spline_json: {\"E\": " << n << ", \"bits\": " << bits << ", \"shift\": " << shift << ", \"degree\": " << d << ", \"runs\": " << runs << ", "
                  << MsJson{"tuples_ms", "tuples_ms_min_max", t_tuples} << ", " << MsJson{"open_ms", "open_ms_min_max", t_open} << ", "
                  << MsJson{"close_ms", "close_ms_min_max", t_close} << "}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("spline mismatch");
}

// threshold decryption end to end (the reference has no local benchmark for it; the calls are the
// ones PartialDecryptionRequestHandler / SMPCClient make, partial_decryption_request_handler.hpp:140,
// smpc_client.hpp:137): share sk t-out-of-n, every party of the first threshold set runs
// part_decrypt_tensor, the combiner runs combine_part_decryption_results_tensor.
static void bench_threshold(const Args &arg) {
    const size_t n = arg(2, 16), m = arg(3, 16), t = arg(4, 2), parties = arg(5, 3);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const auto &pk = fx.pk();
    auto shares = cs.keygen(sk, t, parties);
    // host check of the sharing: for the first threshold set {0..t-1}, s_0 - s_1 - ... - s_(t-1) = sk
    {
        Mpz acc = shares[0][0];
        for (size_t j = 1; j < t; j++) mpz_sub(acc.get(), acc.get(), shares[j][0].get());
        if (!(acc == sk)) throw std::runtime_error("shares do not reconstruct the secret key");
    }
    Owned<PT> pts = plain_tensor(fx, {n, m}, ramp);
    Owned<CT> ct = cs.encrypt_tensor(pk, pts);
    Benchmark bp("part_decrypt_tensor"), bc("combine_part_decryption_results_tensor");
    Vector<Tensor<CS::PartDecryptionResult *>> pdrs;
    bp.run([&]() { pdrs.push_back(cs.part_decrypt_tensor(shares[pdrs.size()][0], ct)); }, (int)t);
    const std::vector<Owned<CS::PartDecryptionResult>> owners(pdrs.begin(), pdrs.end());
    // wire format round trip of the first party's result
    {
        auto bytes = cs.serialize_part_decryption_result_tensor(pdrs[0]);
        Owned<CS::PartDecryptionResult> back = cs.deserialize_part_decryption_result_tensor(bytes);
        if (cs.serialize_part_decryption_result_tensor(back) != bytes) throw std::runtime_error("pdr format round trip");
    }
    bool ok = true;
    bc.run([&]() {
        Owned<PT> res = cs.combine_part_decryption_results_tensor(ct, pdrs);
        if (!matches(cs, res, ramp)) ok = false;
    }, 1);
    bp.print_summary();
    bc.print_summary();
    std::cout << "  threshold " << t << " of " << parties << ": " << (ok ? "ok" : "FAILED") << std::endl;
    std::cout << "n: " << n << " m: " << m << std::endl;
    if (!ok) throw std::runtime_error("threshold decryption mismatch");
}

// the operands of both ciphertext x ciphertext modes
static float beaver_aval(size_t i) { return (float)(i % 7) - 3.0f; }
static float beaver_bval(size_t i) { return (float)(i % 5) + 1.0f; }

// ciphertext x ciphertext matrix product through the Beaver-triplet protocol with an in-process
// client (smpc_local.hpp; reference: SMPCCipherTextMultiplier::multiply_ciphertext_tensors,
// include/smpc/ciphertext_multiplications.hpp:40-112).  threshold = 0: the client decrypts with the
// secret key; otherwise by t-of-n threshold decryption.
static void bench_ciphertext_matmul(const Args &arg) {
    const size_t n = arg(2, 4), m = arg(3, 4), p = arg(4, 4), t = arg(5, 0), parties = arg(6, 3);
    Fixture fx;
    auto &cs = fx.cs;
    auto client = make_client(fx, t, parties);
    Multiplier mul(*client);
    const auto &pk = client->network_public_key();
    Owned<PT> pa = plain_tensor(fx, {n, m}, beaver_aval), pb = plain_tensor(fx, {m, p}, beaver_bval);
    Owned<CT> ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
    Benchmark b("ciphertext_matmul (Beaver triplets, in-process client)");
    bool ok = true;
    b.run([&]() {
        Owned<CT> res = mul.multiply_ciphertext_tensors(ca, cb);
        if (!decrypts_to(fx, res, matmul_reference(n, m, p, beaver_aval, beaver_bval))) ok = false;
    }, 1);
    b.print_summary();
    std::cout << "  " << n * m * p << " element products, " << client->decrypted_elements() << " decryptions (" << client_label(t, parties)
              << "): " << (ok ? "ok" : "FAILED") << std::endl;
    std::cout << "n: " << n << " m: " << m << " p: " << p << std::endl;
    if (!ok) throw std::runtime_error("ciphertext matmul mismatch");
}

// plaintext matrix (n x m) . ciphertext matrix (m x p), the linear layer y = W x: deterministic operands and a fixed Enc(0),
// written to files for the parity checker like the scal_matmul mode (local_bench_lmm_*.bin)
static void bench_plain_ct_matmul(const Args &arg) {
    const size_t n = arg(2, 3), m = arg(3, 5), p = arg(4, 4);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &pk = fx.pk();
    Owned<PT> w = plain_tensor(fx, {n, m}, beaver_aval);       // weights of both signs
    Owned<PT> x = plain_tensor(fx, {m, p}, ramp);
    Owned<CT> cx = cs.encrypt_tensor(pk, x);
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    Benchmark b("plain_ct_matmul (plaintext n x m . ciphertext m x p)");
    std::string out_bytes;
    bool ok = true;
    b.run([&]() {
        Owned<CT> res = cs.matmul_plaintext_ciphertext_tensors(pk, w, cx, &zero);
        out_bytes = cs.serialize_ciphertext_tensor(res);
        if (!decrypts_to(fx, res, matmul_reference(n, m, p, beaver_aval, ramp))) ok = false;
    }, 1);
    b.print_summary();
    write_bytes("local_bench_lmm_s.bin", cs.serialize_plaintext_tensor(w));
    write_ciphertexts(fx, "local_bench_lmm_cts.bin", cx);
    write_ciphertext(fx, "local_bench_lmm_zero.bin", zero);
    write_bytes("local_bench_lmm_out.bin", out_bytes);
    write_absdelta(fx);
    std::cout << "  decrypts to W x: " << (ok ? "yes" : "NO") << std::endl;
    std::cout << "n: " << n << " m: " << m << " p: " << p << std::endl;
    if (!ok) throw std::runtime_error("plaintext-left product mismatch");
}

// plaintext filters kh x kw x C x Co over an encrypted image B x H x W x C (channels last): encrypt, convolve, decrypt and
// compare with the convolution of the plaintexts.  B H W C kh kw Co [sh sw ph pw]; by default stride 1 and "same" padding
static void bench_conv2d(const Args &arg) {
    const size_t kh = arg(6, 3), kw = arg(7, 3);
    const ConvGeometry g{arg(2, 1), arg(3, 6), arg(4, 6), arg(5, 2), kh, kw, arg(8, 2), 1, 1, 1, arg(9, 1), arg(10, 1), arg(11, kh / 2), arg(12, kw / 2)};
    Fixture fx;
    Owned<PT> w = plain_tensor(fx, {g.kh, g.kw, g.C, g.Co}, conv_wval);
    const ConvResult r = conv_check(fx, "conv2d (plaintext filters over a ciphertext image)", g, conv_wval, [&](const CS::PublicKey &pk, const Tensor<CT *> &cx) {
        return fx.cs.conv2d_plaintext_ciphertext_tensors(pk, w, cx, {g.sh, g.sw}, {g.ph, g.pw});
    });
    std::cout << "  decrypts to the convolution: " << (r.ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << g.B << "x" << g.H << "x" << g.W << "x" << g.C << " filters: " << g.kh << "x" << g.kw << "x" << g.C << "x" << g.Co
              << " stride: " << g.sh << "," << g.sw << " pad: " << g.ph << "," << g.pw << " out: " << r.Ho << "x" << r.Wo << std::endl;
    if (!r.ok) throw std::runtime_error("convolution mismatch");
}

// the same with dilation and groups: filters kh x kw x C/G x Co, output column co reads the channels of group co / (Co / G).
// B H W C kh kw Co groups [dh dw sh sw ph pw]; by default no dilation, stride 1 and "same" padding
static void bench_conv2d_grouped(const Args &arg) {
    const size_t kh = arg(6, 3), kw = arg(7, 3), dh = arg(10, 1), dw = arg(11, 1);
    const ConvGeometry g{arg(2, 1), arg(3, 6), arg(4, 6), arg(5, 4), kh, kw, arg(8, 4), arg(9, 4), dh, dw, arg(12, 1), arg(13, 1),
                         arg(14, (kh - 1) * dh / 2), arg(15, (kw - 1) * dw / 2)};
    if (g.groups == 0 || g.C % g.groups || g.Co % g.groups) throw std::invalid_argument("conv2d_grouped: groups must divide C and Co");
    Fixture fx;
    const size_t Cg = g.C / g.groups;
    Owned<PT> w = plain_tensor(fx, {g.kh, g.kw, Cg, g.Co}, conv_wval);
    const ConvResult r = conv_check(fx, "conv2d_grouped (plaintext filters in groups over a ciphertext image)", g, conv_wval,
                                    [&](const CS::PublicKey &pk, const Tensor<CT *> &cx) {
                                        return fx.cs.conv2d_plaintext_ciphertext_tensors(pk, w, cx, {g.sh, g.sw}, {g.ph, g.pw}, {g.dh, g.dw}, g.groups);
                                    });
    std::cout << "  decrypts to the grouped convolution: " << (r.ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << g.B << "x" << g.H << "x" << g.W << "x" << g.C << " filters: " << g.kh << "x" << g.kw << "x" << Cg << "x" << g.Co
              << " groups: " << g.groups << " dilation: " << g.dh << "," << g.dw << " stride: " << g.sh << "," << g.sw << " pad: " << g.ph << "," << g.pw
              << " out: " << r.Ho << "x" << r.Wo << std::endl;
    if (!r.ok) throw std::runtime_error("grouped convolution mismatch");
}

// sum pooling over kh x kw windows of an encrypted image B x H x W x C: encrypt, pool, decrypt and compare with the window sums.
// B H W C kh kw [sh sw ph pw]; by default the stride is the window and there is no padding
static void bench_sum_pool2d(const Args &arg) {
    const size_t C = arg(5, 2), kh = arg(6, 2), kw = arg(7, 2);
    const ConvGeometry g{arg(2, 1), arg(3, 6), arg(4, 6), C, kh, kw, C, C, 1, 1, arg(8, kh), arg(9, kw), arg(10, 0), arg(11, 0)};
    Fixture fx;
    const ConvResult r = conv_check(fx, "sum_pool2d (window sums of a ciphertext image)", g, [](size_t) { return 1.0f; },
                                    [&](const CS::PublicKey &pk, const Tensor<CT *> &cx) {
                                        return fx.cs.sum_pool2d_ciphertext_tensor(pk, cx, {g.kh, g.kw}, {g.sh, g.sw}, {g.ph, g.pw});
                                    });
    std::cout << "  decrypts to the window sums: " << (r.ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << g.B << "x" << g.H << "x" << g.W << "x" << g.C << " window: " << g.kh << "x" << g.kw << " stride: " << g.sh << "," << g.sw
              << " pad: " << g.ph << "," << g.pw << " out: " << r.Ho << "x" << r.Wo << std::endl;
    if (!r.ok) throw std::runtime_error("sum pooling mismatch");
}

// the ciphertext x ciphertext matrix product twice on the same inputs: the reference's expansion into n m p element
// products (2 n m p opened values) and one matrix triplet (LocalCipherTextMultiplier::set_matrix_triplets: n m + m p)
static void bench_ciphertext_matmul_matrix(const Args &arg) {
    const size_t n = arg(2, 4), m = arg(3, 4), p = arg(4, 4), t = arg(5, 0), parties = arg(6, 3);
    Fixture fx;
    auto &cs = fx.cs;
    auto client = make_client(fx, t, parties);
    Multiplier mul(*client);
    const auto &pk = client->network_public_key();
    Owned<PT> pa = plain_tensor(fx, {n, m}, beaver_aval), pb = plain_tensor(fx, {m, p}, beaver_bval);
    Owned<CT> ca = cs.encrypt_tensor(pk, pa), cb = cs.encrypt_tensor(pk, pb);
    bool ok[2] = {true, true};
    double ms[2] = {0, 0};
    size_t opened[2] = {0, 0};
    for (int matrix = 0; matrix < 2; matrix++) {
        mul.set_matrix_triplets(matrix != 0);
        const size_t before = client->decrypted_elements();
        cs.synchronize();
        auto run = timed(cs, [&]() -> Owned<CT> { return mul.multiply_ciphertext_tensors(ca, cb); });
        ms[matrix] = run.first;
        opened[matrix] = client->decrypted_elements() - before;
        ok[matrix] = decrypts_to(fx, run.second, matmul_reference(n, m, p, beaver_aval, beaver_bval));
    }
    std::cout << "  element flow: decrypted_elements " << opened[0] << ", " << ms[0] << " ms: " << (ok[0] ? "ok" : "FAILED") << std::endl;
    std::cout << "  matrix flow: decrypted_elements " << opened[1] << ", " << ms[1] << " ms: " << (ok[1] ? "ok" : "FAILED") << std::endl;
    std::cout << "  (host wall clock, triplet generation and decryptions included; " << client_label(t, parties) << ")" << std::endl;
    std::cout << "  agree: " << (ok[0] && ok[1] ? "yes" : "NO") << std::endl;
    std::cout << "n: " << n << " m: " << m << " p: " << p << std::endl;
    if (!(ok[0] && ok[1])) throw std::runtime_error("ciphertext matmul mismatch");
}

// an encrypted image B x H x W x C under ENCRYPTED filters kh x kw x C x Co (channels last) through one convolution Beaver
// triplet (LocalCipherTextMultiplier::conv2d_ciphertext_tensors): uniform operands in Z/2^k, the result decrypted and compared
// with the exact convolution of the plaintexts mod 2^k; the opened values counted next to what element triplets (2 n m p) and a
// matrix triplet on the patch matrix (n m + m p) would open for the layer.  Also the E * [Bf] term on its own from a fixed
// Enc(0) -- the plaintext image under the encrypted filters, deterministic --, written with its operands for the parity checker
// (local_bench_cconv_*.bin).  B H W C kh kw Co [sh sw ph pw dh dw [t parties [runs]]]; runs > 0: the phases of the flow, timed
static void bench_conv2d_ciphertext(const Args &arg) {
    const ConvGeometry g{arg(2, 1), arg(3, 5), arg(4, 4), arg(5, 2), arg(6, 3), arg(7, 2), arg(8, 2), 1, arg(13, 1), arg(14, 1),
                         arg(9, 1), arg(10, 1), arg(11, 0), arg(12, 0)};
    const size_t t = arg(15, 0), parties = arg(16, 3);
    const int runs = arg.integer(17, 0);
    const std::array<size_t, 2> stride{g.sh, g.sw}, pad{g.ph, g.pw}, dilation{g.dh, g.dw};
    Fixture fx;
    auto &cs = fx.cs;
    const uint32_t k = cs.message_bits();
    auto client = make_client(fx, t, parties);
    Multiplier mul(*client);
    const auto &pk = client->network_public_key();
    auto uniform = [&](size_t) { return cs.random_plaintext(k); };
    Owned<PT> px = plain_tensor(fx, {g.B, g.H, g.W, g.C}, uniform), pw = plain_tensor(fx, {g.kh, g.kw, g.C, g.Co}, uniform);
    Owned<CT> cx = cs.encrypt_tensor(pk, px), cw = cs.encrypt_tensor(pk, pw);
    const size_t before = client->decrypted_elements();
    cs.synchronize();
    auto flow = timed(cs, [&]() -> Owned<CT> { return mul.conv2d_ciphertext_tensors(cx, cw, stride, pad, dilation); });
    const size_t opened = client->decrypted_elements() - before;
    const std::vector<size_t> oshape = flow.second->shape();
    if (oshape.size() != 4 || oshape[0] != g.B || oshape[3] != g.Co) throw std::runtime_error("conv2d_ciphertext: the output is not B x . x . x Co");
    const size_t Ho = oshape[1], Wo = oshape[2], n = g.B * Ho * Wo, m = g.kh * g.kw * g.C, p = g.Co;
    const std::vector<Mpz> want = conv_reference_mod(g, Ho, Wo, px, pw, k);
    const bool flow_ok = decrypts_to(fx, flow.second, want);
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    Owned<CT> term = cs.conv2d_ciphertext_filters_tensors(pk, px, cw, stride, pad, dilation, &zero);
    const bool term_ok = term->shape() == oshape && decrypts_to(fx, term, want);
    write_bytes("local_bench_cconv_img.bin", cs.serialize_plaintext_tensor(px));
    write_bytes("local_bench_cconv_w.bin", cs.serialize_plaintext_tensor(pw));
    write_ciphertexts(fx, "local_bench_cconv_image_cts.bin", cx);
    write_ciphertexts(fx, "local_bench_cconv_filters.bin", cw);
    write_ciphertext(fx, "local_bench_cconv_zero.bin", zero);
    write_ciphertexts(fx, "local_bench_cconv_term.bin", term);
    write_ciphertexts(fx, "local_bench_cconv_out.bin", flow.second);
    write_absdelta(fx);
    std::cout << "  conv flow: decrypted_elements " << opened << ", " << flow.first << " ms: " << (flow_ok ? "ok" : "FAILED") << std::endl;
    std::cout << "  the same layer would open 2 n m p = " << 2 * n * m * p << " values with element triplets, n m + m p = " << n * m + m * p
              << " with a matrix triplet on the patch matrix" << std::endl;
    std::cout << "  plaintext image under the encrypted filters (E * [Bf] alone, from a fixed Enc(0)): " << (term_ok ? "ok" : "FAILED") << std::endl;
    std::cout << "  (host wall clock, triplet generation and decryptions included; " << client_label(t, parties) << ")" << std::endl;
    bool ok = flow_ok && term_ok && opened == px->num_elements() + pw->num_elements();
    if (runs > 0) {
        // the flow phase by phase on the same inputs, spelled as conv2d_ciphertext_tensors spells it, and the whole call; a warm-up
        // pass and `runs` timed ones, medians and extremes on one line
        enum { TRIPLET, OPEN, E_BF, A_D, E_D, TOTAL, PHASES };
        std::vector<double> ms[PHASES];
        for (int pass = 0; pass <= runs; pass++) {
            double at[PHASES];
            cs.synchronize();
            auto trip = timed(cs, [&] { return client->get_beavers_conv2d_triplet(px->shape(), pw->shape(), stride, pad, dilation); });
            Owned<CT> a(trip.second[0]), bf(trip.second[1]), c(trip.second[2]);
            at[TRIPLET] = trip.first;
            auto open = timed(cs, [&] {
                Owned<CT> xa = cs.sub_ciphertext_tensors(pk, cx, a), wb = cs.sub_ciphertext_tensors(pk, cw, bf);
                Owned<PT> e = client->decrypt_tensor(xa);
                return std::make_pair(std::move(e), Owned<PT>(client->decrypt_tensor(wb)));
            });
            at[OPEN] = open.first;
            const Owned<PT> &e = open.second.first, &d = open.second.second;
            auto e_bf = timed(cs, [&]() -> Owned<CT> { return cs.conv2d_ciphertext_filters_tensors(pk, e, bf, stride, pad, dilation); });
            at[E_BF] = e_bf.first;
            auto a_d = timed(cs, [&]() -> Owned<CT> { return cs.conv2d_plaintext_ciphertext_tensors(pk, d, a, stride, pad, dilation, 1); });
            at[A_D] = a_d.first;
            auto e_d = timed(cs, [&]() -> Owned<PT> { return cs.conv2d_plaintext_tensors(e, d, stride, pad, dilation); });
            at[E_D] = e_d.first;
            auto whole = timed(cs, [&]() -> Owned<CT> { return mul.conv2d_ciphertext_tensors(cx, cw, stride, pad, dilation); });
            at[TOTAL] = whole.first;
            if (!decrypts_to(fx, whole.second, want)) ok = false;
            if (pass)
                for (int ph = 0; ph < PHASES; ph++) ms[ph].push_back(at[ph]);
        }
        for (auto &v : ms) std::sort(v.begin(), v.end());
        std::cout << "conv2d_ciphertext_json: {\"image\": [" << g.B << ", " << g.H << ", " << g.W << ", " << g.C << "], \"filters\": [" << g.kh << ", " << g.kw
                  << ", " << g.C << ", " << g.Co << "], \"out\": [" << Ho << ", " << Wo << "], \"runs\": " << runs << ", \"opened\": " << opened << ", "
                  << MsJson{"triplet_ms", "triplet_ms_min_max", ms[TRIPLET]} << ", " << MsJson{"open_ms", "open_ms_min_max", ms[OPEN]} << ", "
                  << MsJson{"e_bf_ms", "e_bf_ms_min_max", ms[E_BF]} << ", " << MsJson{"a_d_ms", "a_d_ms_min_max", ms[A_D]} << ", "
                  << MsJson{"e_d_ms", "e_d_ms_min_max", ms[E_D]} << ", " << MsJson{"total_ms", "total_ms_min_max", ms[TOTAL]} << "}" << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    std::cout << "image: " << g.B << "x" << g.H << "x" << g.W << "x" << g.C << " filters: " << g.kh << "x" << g.kw << "x" << g.C << "x" << g.Co
              << " stride: " << g.sh << "," << g.sw << " pad: " << g.ph << "," << g.pw << " dilation: " << g.dh << "," << g.dw << " out: " << Ho << "x" << Wo
              << std::endl;
    if (!ok) throw std::runtime_error("ciphertext convolution mismatch");
}

// text formats of single values and the binary plaintext-tensor format (cpu_cryptosystem.inl:124-318): written to
// files for the parity checker, and read back
static void bench_formats(const Args &) {
    Fixture fx;
    auto &cs = fx.cs;
    const auto &sk = fx.sk;
    const auto &pk = fx.pk();
    auto ct = cs.encrypt(pk, cs.make_plaintext(42));
    bool ok = true;
    const std::string txt = cs.serialize_ciphertext(ct);
    auto back = cs.deserialize_ciphertext(txt);
    if (!(back.c1() == ct.c1()) || !(back.c2() == ct.c2())) ok = false;
    if (!(cs.deserialize_public_key(cs.serialize_public_key(pk)) == pk)) ok = false;
    if (!(cs.deserialize_secret_key(cs.serialize_secret_key(sk)) == sk)) ok = false;
    auto pd = cs.part_decrypt(sk, ct);
    if (!(cs.deserialize_part_decryption_result(cs.serialize_part_decryption_result(pd)) == pd)) ok = false;
    const float vals[6] = {0.0f, 1.0f, -1.0f, 255.0f, -65536.0f, 123456.0f};
    Owned<PT> pts = plain_tensor(fx, {2, 3}, [&](size_t i) { return vals[i]; });
    const std::string bin = cs.serialize_plaintext_tensor(pts);
    {
        Owned<PT> pb = cs.deserialize_plaintext_tensor(bin);
        if (pb->shape() != pts->shape()) ok = false;
        for (int i = 0; i < 6; i++)
            if (!(*pb[i] == *pts[i])) ok = false;
        if (cs.serialize_plaintext_tensor(pb) != bin) ok = false;
    }
    if (cs.serialize_plaintext(*pts[3]) != "255" || !(cs.deserialize_plaintext("255") == *pts[3])) ok = false;
    write_ciphertext(fx, "local_bench_fmt_ct.bin", ct);
    write_bytes("local_bench_fmt_ct.txt", txt);
    write_bytes("local_bench_fmt_pt.bin", bin);
    {
        std::string lines;
        for (int i = 0; i < 6; i++) lines += cs.serialize_plaintext(*pts[i]) + "\n";
        write_bytes("local_bench_fmt_pt.txt", lines);
    }
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
        auto res = std::make_unique<CT>(x);
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
        // negate_plaintext_tensor keeps the shape
        Owned<PT> np = cs.negate_plaintext_tensor(pts);
        if (np->shape() != pts->shape() || cs.get_float_from_plaintext(*np[3]) != -255.0f) ok = false;
    }
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
static void bench_threads(const Args &arg) {
    const int rounds = arg.integer(2, 4);
    Fixture fx;
    auto &cs = fx.cs;
    const auto &pk = fx.pk();
    const size_t n = 3, m = 4, p = 4;
    Owned<PT> pt1 = plain_tensor(fx, {n, m}, ramp), pt2 = plain_tensor(fx, {m, p}, [](size_t i) { return (float)(i % 5) - 2.0f; });
    Owned<CT> ct1 = cs.encrypt_tensor(pk, pt1);
    auto zero = cs.encrypt(pk, cs.make_plaintext(0));
    Owned<CT> ref = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
    const std::string ref_bytes = cs.serialize_ciphertext_tensor(ref);
    std::atomic<bool> ok{true};
    std::thread ta([&]() {
        for (int r = 0; r < rounds; r++) {
            // alternate shapes so that the workspace is re-sized while the other thread uses the context
            Owned<CT> res = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
            if (cs.serialize_ciphertext_tensor(res) != ref_bytes) ok = false;
        }
    });
    std::thread tb([&]() {
        for (int r = 0; r < rounds; r++)
            if (!decrypts_to(fx, ct1, ramp)) ok = false;
    });
    ta.join();
    tb.join();
    // A shared RESULT tensor read by both threads the way the reference reads it -- through the tensor's non-const element
    // pointers, cts.at(i)->c1() (cpu_cryptosystem_tensor_ops.inl:175; the compute server shares tensors between its 8
    // threads): the non-const accessors must not touch the element's block reference (they used to reset it: a race with
    // the other reader and with copies).  Lazy elements, first touched concurrently; every value compared with a
    // single-threaded const read of a second, identical result.
    {
        Owned<CT> shared = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
        Owned<CT> check = cs.scal_ciphertext_tensors(pk, pt2, ct1, &zero);
        const size_t E = n * p;
        std::vector<std::string> want(E);
        for (size_t i = 0; i < E; i++) {
            const CT &c = *check[i];
            want[i] = c.c1().a().str() + " " + c.c2().b().str();
        }
        auto reader = [&](int start) {
            for (int r = 0; r < rounds; r++)
                for (size_t k = 0; k < E; k++) {
                    const size_t i = (k + start) % E;
                    CT *e = shared[i];                                // non-const, as a Tensor<CipherText *> hands it out
                    CT copy(*e);                                      // copies race with the other thread's first read
                    if (e->c1().a().str() + " " + e->c2().b().str() != want[i]) ok = false;
                    if (copy.c1().a().str() + " " + copy.c2().b().str() != want[i]) ok = false;
                }
        };
        std::thread r1(reader, 0), r2(reader, (int)(E / 2));
        r1.join();
        r2.join();
        // a touched element no longer offers its device copy; the values are still what the block holds
        for (size_t i = 0; i < E; i++)
            if (shared[i]->block()) ok = false;
    }
    std::cout << "  two threads on one cryptosystem, " << rounds << " rounds each: " << (ok ? "ok" : "FAILED") << std::endl;
    if (!ok) throw std::runtime_error("concurrent use gave a different result");
}

// make_plaintext / get_float_from_plaintext of the product on floats given by their bit patterns (one 8-digit hex word
// per line of `in`): "<decimal plaintext> <bit pattern of the float that comes back>" per line of `out`
static void plaintexts_mode(const Args &arg) {
    if (arg.argc < 4) throw std::invalid_argument("plaintexts <in> <out>");
    Fixture fx;
    std::ifstream fi(arg.argv[2]);
    std::ofstream fo(arg.argv[3]);
    std::string tok;
    while (fi >> tok) {
        const uint32_t bits = (uint32_t)std::stoul(tok, nullptr, 16);
        float x;
        memcpy(&x, &bits, 4);
        auto pt = fx.cs.make_plaintext(x);
        const float back = fx.cs.get_float_from_plaintext(pt);
        uint32_t bb;
        memcpy(&bb, &back, 4);
        char buf[16];
        snprintf(buf, sizeof buf, "%08x", bb);
        fo << pt.str() << " " << buf << "\n";
    }
}

// Rearranging resident tensors (view_ciphertext_tensor and kin, the device route of upload): an image of distinct small values
// is encrypted, and everything below runs on the RESULT of add_ciphertext_tensors(x, x), a resident block -- a permutation of the
// axes, a slice with a negative step, a padding, a broadcast, a concatenation with a flipped copy, the window taps of the
// geometry and an index gather; then the three columns of an [n, 3] block through upload, and max_pool2d with the geometry's
// padding on 4-bit values.  Prints block_downloads (the record downloads before the first decryption: 0 when nothing left the
// device), decrypts everything, compares with host loops and prints "<name> ok" per operation; last, the upload of the three
// columns of a 4096 x 3 block with the device route on and off (medians over fresh blocks).
static void bench_rearrange(const Args &arg) {
    const size_t B = arg(2, 1), H = arg(3, 5), W = arg(4, 4), C = arg(5, 2), kh = arg(6, 3), kw = arg(7, 2);
    const size_t sh = arg(8, 2), sw = arg(9, 1), ph = arg(10, 1), pw = arg(11, 1), dh = arg(12, 1), dw = arg(13, 1);
    Fixture fx;
    auto &cs = fx.cs;
    Client client(cs, fx.sk);
    Multiplier mul(client);
    const auto &pk = client.network_public_key();
    const size_t n = B * H * W * C;
    auto val = [](size_t i) { return (float)((i * 5) % 15) - 7.0f; };          // within 4 bits, signed; x + x doubles it
    auto v2 = [&](size_t i) { return 2.0f * val(i); };
    auto at = [&](size_t b, size_t y, size_t x, size_t c) { return ((b * H + y) * W + x) * C + c; };
    const float FILLV = 99.0f;
    Owned<PT> px = plain_tensor(fx, {B, H, W, C}, val);
    Owned<CT> cx = cs.encrypt_tensor(pk, px);
    Owned<CT> r = cs.add_ciphertext_tensors(pk, cx, cx);
    const CT fill = cs.encrypt(pk, cs.make_plaintext(FILLV));
    const uint64_t downloads0 = cs.block_downloads();

    struct Case {
        std::string name;
        Owned<CT> got;
        std::vector<float> want;
        std::vector<size_t> shape;
    };
    std::vector<Case> cases;
    {   // permute by (3, 1, 0, 2): [C, H, B, W]
        std::vector<float> w;
        for (size_t c = 0; c < C; c++) for (size_t y = 0; y < H; y++) for (size_t b = 0; b < B; b++) for (size_t x = 0; x < W; x++) w.push_back(v2(at(b, y, x, c)));
        cases.push_back({"permute", cs.permute_ciphertext_tensor(r, {3, 1, 0, 2}), w, {C, H, B, W}});
    }
    {   // rows H - 1, H - 3, ..: a negative step down to and including row 0
        std::vector<float> w;
        size_t rows = 0;
        for (size_t b = 0; b < B; b++) {
            rows = 0;
            for (long y = (long)H - 1; y >= 0; y -= 2, rows++) for (size_t x = 0; x < W; x++) for (size_t c = 0; c < C; c++) w.push_back(v2(at(b, (size_t)y, x, c)));
        }
        cases.push_back({"slice", cs.slice_ciphertext_tensor(r, {0, (int64_t)H - 1, 0, 0}, {(int64_t)B, -1, (int64_t)W, (int64_t)C}, {1, -2, 1, 1}), w, {B, rows, W, C}});
    }
    {   // one row above, two columns left and one right
        std::vector<float> w;
        for (size_t b = 0; b < B; b++) for (size_t y = 0; y < H + 1; y++) for (size_t x = 0; x < W + 3; x++) for (size_t c = 0; c < C; c++)
            w.push_back(y >= 1 && x >= 2 && x < W + 2 ? v2(at(b, y - 1, x - 2, c)) : FILLV);
        cases.push_back({"pad", cs.pad_ciphertext_tensor(r, {0, 1, 2, 0}, {0, 0, 1, 0}, fill), w, {B, H + 1, W + 3, C}});
    }
    {   // three copies along a new leading axis
        std::vector<float> w;
        for (size_t rep = 0; rep < 3; rep++) for (size_t i = 0; i < n; i++) w.push_back(v2(i));
        cases.push_back({"broadcast", cs.broadcast_ciphertext_tensor(r, {3, B, H, W, C}), w, {3, B, H, W, C}});
    }
    {   // the image and its mirror side by side along W
        Owned<CT> mirror = cs.flip_ciphertext_tensor(r, 2);
        std::vector<float> w;
        for (size_t b = 0; b < B; b++) for (size_t y = 0; y < H; y++) for (size_t x = 0; x < 2 * W; x++) for (size_t c = 0; c < C; c++)
            w.push_back(v2(at(b, y, x < W ? x : 2 * W - 1 - x, c)));
        cases.push_back({"concat", cs.concat_ciphertext_tensors({r, mirror}, 2), w, {B, H, 2 * W, C}});
    }
    size_t Ho = 0, Wo = 0;
    {
        Owned<CT> taps = cs.window_taps_ciphertext_tensor(r, {kh, kw}, {sh, sw}, {ph, pw}, {dh, dw}, &fill);
        if (taps->shape().size() != 6) throw std::runtime_error("window taps: not 6-D");
        Ho = taps->shape()[3];
        Wo = taps->shape()[4];
        std::vector<float> w;
        for (size_t dy = 0; dy < kh; dy++) for (size_t dx = 0; dx < kw; dx++) for (size_t b = 0; b < B; b++) for (size_t oy = 0; oy < Ho; oy++)
            for (size_t ox = 0; ox < Wo; ox++) for (size_t c = 0; c < C; c++) {
                const long y = (long)(oy * sh + dy * dh) - (long)ph, x = (long)(ox * sw + dx * dw) - (long)pw;
                w.push_back(y >= 0 && y < (long)H && x >= 0 && x < (long)W ? v2(at(b, (size_t)y, (size_t)x, c)) : FILLV);
            }
        cases.push_back({"window_taps", std::move(taps), w, {kh, kw, B, Ho, Wo, C}});
    }
    {   // the elements backwards, every fifth one the fill
        std::vector<uint32_t> idx(n);
        std::vector<float> w(n);
        for (size_t i = 0; i < n; i++) {
            idx[i] = i % 5 == 4 ? COFHE_HIP_GATHER_FILL : (uint32_t)(n - 1 - i);
            w[i] = i % 5 == 4 ? FILLV : v2(n - 1 - i);
        }
        cases.push_back({"gather", cs.gather_ciphertext_tensor(r, idx, &fill), w, {n}});
    }
    // the columns of an [n, 3] block, as the Beaver flows split a triplet block: pointers into one resident block, through upload
    Owned<PT> p3 = plain_tensor(fx, {n, 3}, val);
    Owned<CT> c3 = cs.encrypt_tensor(pk, p3);
    Owned<CT> r3 = cs.add_ciphertext_tensors(pk, c3, c3);
    auto column = [](const Tensor<CT *> &block, size_t rows, size_t j) {
        Tensor<CT *> col(rows, nullptr);
        for (size_t i = 0; i < rows; i++) col[i] = block[i * 3 + j];
        return col;
    };
    for (size_t j = 0; j < 3; j++) {
        std::vector<float> w;
        for (size_t i = 0; i < n; i++) w.push_back(v2(i * 3 + j));
        cases.push_back({"column_split_" + std::to_string(j), cs.download(cs.upload(column(r3, n, j))), w, {n}});
    }
    std::cout << "block_downloads=" << cs.block_downloads() - downloads0 << std::endl;

    bool ok = true;
    for (const Case &c : cases) {
        const bool pass = c.got->shape() == c.shape && decrypts_to(fx, c.got, c.want);
        std::cout << c.name << " " << (pass ? "ok" : "FAILED") << std::endl;
        ok = ok && pass;
    }
    {   // max pooling with the geometry's padding on the 4-bit image itself; the least value stands in the padding
        const uint32_t bits = 4;
        Owned<CT> pooled = mul.max_pool2d_ciphertext_tensor(cx, {kh, kw}, {sh, sw}, bits, {ph, pw});
        const size_t Hp = (H + 2 * ph - kh) / sh + 1, Wp = (W + 2 * pw - kw) / sw + 1;
        std::vector<float> w;
        for (size_t b = 0; b < B; b++) for (size_t oy = 0; oy < Hp; oy++) for (size_t ox = 0; ox < Wp; ox++) for (size_t c = 0; c < C; c++) {
            float m = -8.0f;
            for (size_t dy = 0; dy < kh; dy++) for (size_t dx = 0; dx < kw; dx++) {
                const long y = (long)(oy * sh + dy) - (long)ph, x = (long)(ox * sw + dx) - (long)pw;
                if (y >= 0 && y < (long)H && x >= 0 && x < (long)W) m = std::max(m, val(at(b, (size_t)y, (size_t)x, c)));
            }
            w.push_back(m);
        }
        const bool pass = pooled->shape() == std::vector<size_t>{B, Hp, Wp, C} && decrypts_to(fx, pooled, w);
        std::cout << "max_pool2d_padded " << (pass ? "ok" : "FAILED") << std::endl;
        ok = ok && pass;
    }
    {   // the device route against the host route: both give the same bytes
        Tensor<CT *> col = column(r3, n, 1);
        Owned<CT> dev = cs.download(cs.upload(col));
        cs.set_resident_gather(false);
        Owned<CT> host = cs.download(cs.upload(col));
        cs.set_resident_gather(true);
        const bool pass = cs.serialize_ciphertext_tensor(dev) == cs.serialize_ciphertext_tensor(host);
        std::cout << "routes_agree " << (pass ? "ok" : "FAILED") << std::endl;
        ok = ok && pass;
    }
    {   // the three columns of a 4096 x 3 block, a fresh block for every pass so that the host route pays its download each time
        const size_t rows = 4096;
        const int runs = 5;
        Owned<PT> pbig = plain_tensor(fx, {rows, 3}, val);
        Owned<CT> cbig = cs.encrypt_tensor(pk, pbig);
        Owned<CT> block;
        auto fresh_block = [&]() { block = cs.add_ciphertext_tensors(pk, cbig, cbig); };
        auto split = [&]() -> Tensor<CT *> {
            for (size_t j = 0; j < 2; j++) (void)cs.upload(column(block, rows, j));
            return cs.download(cs.upload(column(block, rows, 2)));
        };
        const auto dev_ms = median_runs(cs, runs, split, fresh_block);
        cs.set_resident_gather(false);
        const auto host_ms = median_runs(cs, runs, split, fresh_block);
        cs.set_resident_gather(true);
        std::cout << "upload_ms device=" << median(dev_ms) << " host=" << median(host_ms) << " (4096 x 3 block, three columns, medians of " << runs
                  << " runs; device [" << dev_ms.front() << ", " << dev_ms.back() << "] host [" << host_ms.front() << ", " << host_ms.back() << "])"
                  << std::endl;
    }
    std::cout << "  agree: " << (ok ? "yes" : "NO") << std::endl;
    if (!ok) throw std::runtime_error("rearrange mismatch");
}

// every mode: its name, its arguments with their defaults, its function
static const struct Mode {
    const char *name, *synopsis;
    void (*run)(const Args &);
} MODES[] = {
    {"encrypt_decrypt", "[n=64 m=64]", bench_encrypt_decrypt},
    {"ciphertext_matadd", "[n=64 m=64]", bench_matadd},
    {"scal_matmul", "[n=8 m=64 p=64 [chain=50]]", bench_scal_matmul},
    {"threshold", "[n=16 m=16 t=2 parties=3]", bench_threshold},
    {"ciphertext_matmul", "[n=4 m=4 p=4 [t=0 parties=3]]", bench_ciphertext_matmul},
    {"ciphertext_matmul_matrix", "[n=4 m=4 p=4 [t=0 parties=3]]", bench_ciphertext_matmul_matrix},
    {"plain_ct_matmul", "[n=3 m=5 p=4]", bench_plain_ct_matmul},
    {"fresh_randomness", "[elements=256]", bench_fresh_randomness},
    {"affine", "[elements=64]", bench_affine},
    {"beaver_direct", "[elements=8]", bench_beaver_direct},
    {"conv2d", "[B=1 H=6 W=6 C=2 kh=3 kw=3 Co=2 [sh=1 sw=1 ph=kh/2 pw=kw/2]]", bench_conv2d},
    {"conv2d_grouped", "[B=1 H=6 W=6 C=4 kh=3 kw=3 Co=4 groups=4 [dh=1 dw=1 sh=1 sw=1 ph=(kh-1)*dh/2 pw=(kw-1)*dw/2]]", bench_conv2d_grouped},
    {"sum_pool2d", "[B=1 H=6 W=6 C=2 kh=2 kw=2 [sh=kh sw=kw ph=0 pw=0]]", bench_sum_pool2d},
    {"conv2d_ciphertext", "[B=1 H=5 W=4 C=2 kh=3 kw=2 Co=2 [sh=1 sw=1 ph=0 pw=0 dh=1 dw=1 [t=0 parties=3 [runs=0]]]]", bench_conv2d_ciphertext},
    {"poly_activation", "[elements=64 [runs=0]]", bench_poly_activation},
    {"divide", "[elements=64 [runs=0]]", bench_divide},
    {"divide_exact", "[elements=64 [runs=0]]", bench_divide_exact},
    {"lookup", "[elements=64 [runs=0]]", bench_lookup},
    {"compare", "[elements=256 [bits=32 [digit_bits=0 [runs=0]]]]", bench_compare},
    {"spline", "[elements=256 [runs=0 [bits=5 [shift=11 [degree=2]]]]]", bench_spline},
    {"rearrange", "[B=1 H=5 W=4 C=2 kh=3 kw=2 [sh=2 sw=1 ph=1 pw=1 dh=1 dw=1]]", bench_rearrange},
    {"formats", "", bench_formats},
    {"threads", "[rounds=4]", bench_threads},
    {"plaintexts", "<in> <out>", plaintexts_mode},
};

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "Usage: " << argv[0] << " <mode> [arguments]" << std::endl;
        for (const Mode &m : MODES) std::cerr << "  " << m.name << (*m.synopsis ? " " : "") << m.synopsis << std::endl;
        return 1;
    }
    const std::string name = argv[1];
    const Mode *mode = std::find_if(std::begin(MODES), std::end(MODES), [&](const Mode &m) { return name == m.name; });
    if (mode == std::end(MODES)) {
        std::cerr << "Invalid benchmark type" << std::endl;
        return 1;
    }
    try {
        mode->run(Args{argc, argv});
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
