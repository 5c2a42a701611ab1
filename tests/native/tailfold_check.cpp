// tests/native/tailfold_check.cpp -- host check of the folded FP64 tail (sunscreen_amd/csrc/moddown_d.hpp tail_fold4_d: the tails' two
// inverse stages with the fixed scaling folded into the stage constants, five constant products instead of eight) and of the
// floor's single product by q^-1 * (B/B_j)^-1, against 128-bit integer arithmetic.  The device code is IEEE double arithmetic
// (fma, add, rint) on both sides: exactness is a property of the arithmetic.  Prints "ok <cases>" or a failure.
//
// Bounds, from the range plan (context.cpp plan_f64_split), not from what the code gives:
//   * a product's argument is at most the four-input sum, which the plan keeps below 0.98 * 2^53 (`limit`): the tail is entered
//     with |v| <= 0.98 * 2^51 at the most (regime WIDE; kPlanScaleReduce set: the kernels reduce every output);
//   * without kPlanScaleReduce the four-input sum M satisfies M * 1.02 / 2^52 <= 0.45 (regime PLAIN): the tail is entered with
//     |v| <= 0.45 / 1.02 * 2^50, every product stays below 0.95 q, so the one output that is a sum of two products is within 2q
//     (what mod_down_d accepts) and one reduction makes it |.| <= q/2 (+1).
//   * a constant product leaves |r| <= q * (0.5 + |y| * 2^-52 * 1.02) (+1) for an argument y (ArithD::mul_const).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "moddown_d.hpp"

typedef unsigned long long u64;
typedef __int128 i128;
using hipbfv::MulOpD;
using hipbfv::TailFoldD;

static u64 mulmod(u64 a, u64 b, u64 m) { return (u64)((unsigned __int128)a * b % m); }
static u64 powmod(u64 a, u64 e, u64 m) {
  u64 r = 1;
  for (a %= m; e; e >>= 1, a = mulmod(a, a, m))
    if (e & 1) r = mulmod(r, a, m);
  return r;
}
static u64 invmod(u64 a, u64 m) { return powmod(a % m, m - 2, m); }
static bool is_prime(u64 n) {
  if (n < 4) return n > 1;
  if (!(n & 1)) return false;
  u64 d = n - 1;
  int s = 0;
  while (!(d & 1)) d >>= 1, s++;
  for (u64 a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
    if (a % n == 0) continue;
    u64 x = powmod(a, d, n);
    if (x == 1 || x == n - 1) continue;
    bool comp = true;
    for (int i = 1; i < s && comp; i++) {
      x = mulmod(x, x, n);
      if (x == n - 1) comp = false;
    }
    if (comp) return false;
  }
  return true;
}
// the largest prime == 1 (mod two_n) not above v
static u64 ntt_prime_below(u64 v, u64 two_n) {
  u64 c = v / two_n * two_n + 1;
  if (c > v) c -= two_n;
  while (!is_prime(c)) c -= two_n;
  return c;
}
// a primitive 2n-th root of unity mod q
static u64 root_2n(u64 q, u64 two_n, std::mt19937_64& rng) {
  for (;;) {
    const u64 g = powmod(rng() % (q - 2) + 2, (q - 1) / two_n, q);
    if (powmod(g, two_n / 2, q) == q - 1) return g;
  }
}
static u64 canon(i128 v, u64 q) { return (u64)((v % (i128)q + (i128)q) % (i128)q); }
static u64 canon_d(double v, u64 q) { return canon((i128)(long long)v, q); }

// as context.cpp make_mulop_d
static MulOpD mulop_d(u64 w, u64 q) {
  MulOpD m;
  m.w = (double)w;
  m.wq = (double)w / (double)q;
  return m;
}

struct Consts {
  u64 q, tw1, tw2, tw3, sc;
  TailFoldD f;
};
static Consts make_consts(u64 q, u64 n, u64 sc, std::mt19937_64& rng) {
  Consts c;
  c.q = q;
  const u64 ipsi = invmod(root_2n(q, 2 * n, rng), q);
  // tw_inv[k] = ipsi^bitrev(k): k = 1, 2, 3 -> n/2, n/4, 3n/4
  c.tw1 = powmod(ipsi, n / 2, q), c.tw2 = powmod(ipsi, n / 4, q), c.tw3 = powmod(ipsi, 3 * n / 4, q);
  c.sc = sc % q;
  c.f.sc = mulop_d(c.sc, q);
  c.f.tw1sc = mulop_d(mulmod(c.tw1, c.sc, q), q);
  c.f.tw2sc = mulop_d(mulmod(c.tw2, c.sc, q), q);
  c.f.tw3sc = mulop_d(mulmod(c.tw3, c.sc, q), q);
  c.f.tw1 = mulop_d(c.tw1, q);
  return c;
}

static long long g_total = 0;

static double reduce_d(double v, double q) { return hipbfv::md_reduce(v, q, 1.0 / q); }

// one tail on v[0..3]; wide: the regime in which the kernels reduce every output
static bool check_tail(const Consts& c, const long long (&vin)[4], bool wide) {
  const u64 q = c.q;
  const double qd = (double)q;
  // the unfolded tail in integers: two Gentleman-Sande stages, then the scaling
  const i128 v0 = vin[0], v1 = vin[1], v2 = vin[2], v3 = vin[3];
  const u64 a0 = canon(v0 + v1, q), a1 = mulmod(canon(v0 - v1, q), c.tw2, q);
  const u64 a2 = canon(v2 + v3, q), a3 = mulmod(canon(v2 - v3, q), c.tw3, q);
  const u64 want[4] = {mulmod((a0 + a2) % q, c.sc, q), mulmod((a1 + a3) % q, c.sc, q), mulmod(mulmod((a0 + q - a2) % q, c.tw1, q), c.sc, q),
                       mulmod(mulmod((a1 + q - a3) % q, c.tw1, q), c.sc, q)};
  double v[4] = {(double)vin[0], (double)vin[1], (double)vin[2], (double)vin[3]};
  // the two first-stage products on their own, for their bounds (the same calls tail_fold4_d makes)
  const double y1 = hipbfv::md_mul_const(v[0] - v[1], c.f.tw2sc.w, c.f.tw2sc.wq, qd);
  const double y3 = hipbfv::md_mul_const(v[2] - v[3], c.f.tw3sc.w, c.f.tw3sc.wq, qd);
  const double arg[4] = {(v[0] + v[1]) + (v[2] + v[3]), 0.0, (v[0] + v[1]) - (v[2] + v[3]), y1 - y3};
  hipbfv::tail_fold4_d(qd, c.f, v);
  auto fail = [&](const char* what, int k) {
    std::printf("FAIL %s k=%d q=%llu sc=%llu v=(%lld %lld %lld %lld) got=(%.1f %.1f %.1f %.1f) want=(%llu %llu %llu %llu)\n", what, k, q, c.sc, vin[0],
                vin[1], vin[2], vin[3], v[0], v[1], v[2], v[3], want[0], want[1], want[2], want[3]);
    return false;
  };
  auto prod_bound = [&](double y) { return qd * (0.5 + std::fabs(y) * 1.02 / 4503599627370496.0) + 1.0; };
  if (v[1] != y1 + y3) return fail("out1 is not the sum of the two first-stage products", 1);
  if (std::fabs(y1) > prod_bound(vin[0] - (double)vin[1]) || std::fabs(y3) > prod_bound(vin[2] - (double)vin[3])) return fail("first-stage product bound", 1);
  for (int k = 0; k < 4; k++) {
    if (v[k] != (double)(long long)v[k]) return fail("not an integer", k);
    if (canon_d(v[k], q) != want[k]) return fail("residue", k);
    if (k != 1 && std::fabs(v[k]) > prod_bound(arg[k])) return fail("product bound", k);
  }
  if (!wide) {
    // kPlanScaleReduce clear: products below 0.95 q, so one conditional add makes them canonical; the sum output within 2q, and
    // canonical after one reduction and one conditional add
    if (std::fabs(y1) >= 0.95 * qd || std::fabs(y3) >= 0.95 * qd) return fail("first-stage product above 0.95 q", 1);
    for (int k = 0; k < 4; k++) {
      if (k != 1 && std::fabs(v[k]) >= 0.95 * qd) return fail("product above 0.95 q", k);
      if (k != 1 && (u64)(v[k] < 0.0 ? v[k] + qd : v[k]) != want[k]) return fail("one conditional add", k);
    }
    if (std::fabs(v[1]) > 2.0 * qd) return fail("|out1| > 2q", 1);
  }
  // every output after the reduction the kernels apply (always to out1 where a canonical value is formed; to all under the flag)
  for (int k = 0; k < 4; k++) {
    const double r = reduce_d(v[k], qd);
    if (std::fabs(r) > 0.5 * qd + 1.0) return fail("reduced output above q/2", k);
    const double cv = r < 0.0 ? r + qd : r;
    if (cv < 0.0 || cv >= qd || (u64)cv != want[k]) return fail("canonical", k);
  }
  g_total++;
  return true;
}

// y with |y| <= bound, y == r (mod q), as close to sign * bound as the residue allows
static long long rep_near(u64 r, u64 q, long long bound, int sign) {
  const long long k = (bound - (long long)q) / (long long)q;  // r + k q <= bound
  long long y = sign > 0 ? (long long)r + k * (long long)q : (long long)r - (k + 1) * (long long)q;
  if (y > bound) y -= (long long)q;
  if (y < -bound) y += (long long)q;
  return y;
}

static bool run_tail_cases(const Consts& c, std::mt19937_64& rng, int trials) {
  const u64 q = c.q;
  // entry bounds of the two regimes (header comment); a prime so wide that PLAIN would enter below q/2 + 1 has no PLAIN regime
  // (the plan sets kPlanScaleReduce for it)
  const long long wide_b = (long long)(0.98 * 2251799813685248.0);
  const long long plain_b = (long long)(0.45 / 1.02 * 1125899906842624.0);
  for (int regime = 0; regime < 2; regime++) {
    const bool wide = regime == 1;
    const long long B = wide ? wide_b : plain_b;
    if (!wide && B < (long long)(q / 2 + 1)) continue;
    auto rnd = [&]() { return (long long)(rng() % (2 * (u64)B + 1)) - B; };
    const u64 targets[5] = {0, 1, q - 1, (q - 1) / 2, (q + 1) / 2};
    for (int trial = 0; trial < trials; trial++) {
      long long v[4] = {rnd(), rnd(), rnd(), rnd()};
      const int mode = trial % 16;
      if (mode == 1) v[0] = v[1] = v[2] = v[3] = B;                  // the largest sum
      if (mode == 2) v[0] = v[1] = v[2] = v[3] = -B;
      if (mode == 3) v[0] = B, v[1] = -B, v[2] = B, v[3] = -B;       // the largest first-stage differences
      if (mode == 4) v[0] = B, v[1] = B, v[2] = -B, v[3] = -B;       // the largest second-stage difference
      if (mode == 5) v[0] = -B, v[1] = B, v[2] = B, v[3] = -B;       // first-stage products of opposite sign
      if (mode >= 6 && mode <= 9) {
        // put one product on 0, +-1, (q +- 1)/2 (mod q): y * w == target for the product's constant w, y near +- its bound
        const u64 target = targets[(trial / 16) % 5];
        const int sign = (trial / 80) % 2 ? 1 : -1;
        if (mode == 6) {  // out0 = (v0 + v1 + v2 + v3) * sc
          const u64 r = mulmod(target, invmod(c.sc, q), q);
          v[1] = sign * (B - (long long)(rng() % q)), v[2] = sign * (B - (long long)(rng() % q)), v[3] = sign * (B - (long long)(rng() % q));
          const long long y = rep_near(r, q, 4 * B, sign);
          v[0] = y - v[1] - v[2] - v[3];
          while (v[0] > B) v[0] -= (long long)q;
          while (v[0] < -B) v[0] += (long long)q;
        } else if (mode == 7) {  // Y1 = (v0 - v1) * tw2 sc
          const u64 r = mulmod(target, invmod(mulmod(c.tw2, c.sc, q), q), q);
          const long long y = rep_near(r, q, 2 * B, sign);
          v[1] = -sign * (B - (long long)(rng() % q));
          v[0] = y + v[1];
          while (v[0] > B) v[0] -= (long long)q;
          while (v[0] < -B) v[0] += (long long)q;
        } else if (mode == 8) {  // out2 = (v0 + v1 - v2 - v3) * tw1 sc
          const u64 r = mulmod(target, invmod(mulmod(c.tw1, c.sc, q), q), q);
          v[1] = sign * (B - (long long)(rng() % q)), v[2] = -sign * (B - (long long)(rng() % q)), v[3] = -sign * (B - (long long)(rng() % q));
          const long long y = rep_near(r, q, 4 * B, sign);
          v[0] = y - v[1] + v[2] + v[3];
          while (v[0] > B) v[0] -= (long long)q;
          while (v[0] < -B) v[0] += (long long)q;
        } else {  // out3 = (Y1 - Y3) * tw1: v0 - v1 == (target / tw1 + (v2 - v3) tw3 sc) / (tw2 sc)
          const u64 y3 = mulmod(canon((i128)v[2] - v[3], q), mulmod(c.tw3, c.sc, q), q);
          const u64 d = mulmod((mulmod(target, invmod(c.tw1, q), q) + y3) % q, invmod(mulmod(c.tw2, c.sc, q), q), q);
          const long long y = rep_near(d, q, 2 * B, sign);
          v[1] = -sign * (B - (long long)(rng() % q));
          v[0] = y + v[1];
          while (v[0] > B) v[0] -= (long long)q;
          while (v[0] < -B) v[0] += (long long)q;
        }
      }
      if (mode == 10) v[0] = v[1], v[2] = v[3];  // zero differences
      if (mode == 11) v[0] = v[1] = v[2] = v[3] = 0;
      for (int k = 0; k < 4; k++)
        if (v[k] > B || v[k] < -B) {
          std::printf("FAIL the test's own operand is out of range\n");
          return false;
        }
      if (!check_tail(c, v, wide)) return false;
    }
  }
  return true;
}

// the floor: fl -> canonical(fl * q^-1 * (B/B_j)^-1), one product against two, for |fl| <= p/2 + 1 (a reduced value)
static bool run_floor_cases(u64 p, u64 invq, u64 ip, std::mt19937_64& rng, int trials) {
  const double pd = (double)p;
  const MulOpD a = mulop_d(invq, p), b = mulop_d(ip, p), ab = mulop_d(mulmod(invq, ip, p), p);
  const u64 w = mulmod(invq, ip, p);
  const u64 targets[5] = {0, 1, p - 1, (p - 1) / 2, (p + 1) / 2};
  const long long H = (long long)(p / 2) + 1;
  for (int trial = 0; trial < trials; trial++) {
    long long y = (long long)(rng() % (2 * (u64)H + 1)) - H;
    const int mode = trial % 8;
    if (mode == 1) y = H;
    if (mode == 2) y = -H;
    if (mode == 3) y = 0;
    if (mode == 4 || mode == 5) {  // the single product lands on 0, +-1, (p +- 1)/2
      const u64 r = mulmod(targets[(trial / 8) % 5], invmod(w, p), p);
      y = (long long)r;
      if (y > H) y -= (long long)p;
    }
    if (mode == 6) {  // the FIRST of the two products lands on such a value
      const u64 r = mulmod(targets[(trial / 8) % 5], invmod(invq, p), p);
      y = (long long)r;
      if (y > H) y -= (long long)p;
    }
    const double one = hipbfv::md_mul_const((double)y, ab.w, ab.wq, pd);
    const double two = hipbfv::md_mul_const(hipbfv::md_mul_const((double)y, a.w, a.wq, pd), b.w, b.wq, pd);
    const double r1 = reduce_d(one, pd), r2 = reduce_d(two, pd);
    const double c1 = r1 < 0.0 ? r1 + pd : r1, c2 = r2 < 0.0 ? r2 + pd : r2;
    const u64 want = mulmod(canon(y, p), w, p);
    if (std::fabs(one) > pd * (0.5 + std::fabs((double)y) * 1.02 / 4503599627370496.0) + 1.0 || c1 != c2 || c1 < 0.0 || c1 >= pd || (u64)c1 != want) {
      std::printf("FAIL floor p=%llu y=%lld one=%.1f two=%.1f want=%llu\n", p, y, one, two, want);
      return false;
    }
    g_total++;
  }
  return true;
}

int main() {
  std::mt19937_64 rng(0x7A11F01Du);
  // (1) primes of 36 ... 50 bits, == 1 (mod 2n) for n = 16384: top, bottom and inside of their size class; the scale kinds are n^-1 and
  // two further constants of the form the BEHZ scalings have (n^-1 * t * x^-1 for a random unit x), t a 17-bit plain modulus
  {
    const u64 n = 16384, t = 114689;
    for (int bits = 36; bits <= 50; bits++) {
      for (int which = 0; which < 3; which++) {
        const u64 top = (1ull << bits) - 1, bot = (1ull << (bits - 1)) + 1;
        const u64 q = ntt_prime_below(which == 0 ? top : which == 1 ? bot + 40 * 2 * n : bot + 2 * n + rng() % (top - bot - 2 * n), 2 * n);
        const u64 ninv = invmod(n, q);
        const u64 kinds[3] = {ninv, mulmod(ninv, t % q, q), mulmod(mulmod(ninv, t % q, q), invmod(rng() % (q - 1) + 1, q), q)};
        for (u64 sc : kinds)
          if (!run_tail_cases(make_consts(q, n, sc, rng), rng, 3200)) return 1;
        const u64 invq = rng() % (q - 1) + 1, ip = rng() % (q - 1) + 1;
        if (!run_floor_cases(q, invq, ip, rng, 8000)) return 1;
      }
    }
  }
  // (2) the n = 8192 default context (SEAL's 218-bit coefficient modulus, t = the 17-bit batching prime): the four data primes,
  // the special prime and the library's five auxiliary primes (B_0 .. B_3, m_sk), each with the constants context.cpp builds
  {
    const u64 n = 8192, t = TAILFOLD_T;
    const std::vector<u64> key = {TAILFOLD_KEY};
    const std::vector<u64> B = {TAILFOLD_B};
    const u64 msk = TAILFOLD_MSK;
    const size_t K = key.size() - 1;
    for (size_t i = 0; i < key.size(); i++) {
      const u64 q = key[i], ninv = invmod(n, q);
      if (!run_tail_cases(make_consts(q, n, ninv, rng), rng, 20000)) return 1;  // key switch: n^-1
      if (i < K) {                                                                // multiply, data row: n^-1 t (q/q_i)^-1
        u64 punct = 1;
        for (size_t k = 0; k < K; k++)
          if (k != i) punct = mulmod(punct, key[k] % q, q);
        if (!run_tail_cases(make_consts(q, n, mulmod(mulmod(ninv, t % q, q), invmod(punct, q), q), rng), rng, 20000)) return 1;
      }
    }
    std::vector<u64> bsk = B;
    bsk.push_back(msk);
    for (size_t j = 0; j < bsk.size(); j++) {
      const u64 p = bsk[j];
      if (!run_tail_cases(make_consts(p, n, mulmod(invmod(n, p), t % p, p), rng), rng, 20000)) return 1;  // auxiliary row: n^-1 t
      if (j < B.size()) {
        u64 qm = 1, punct = 1;
        for (size_t k = 0; k < K; k++) qm = mulmod(qm, key[k] % p, p);
        for (size_t k = 0; k < B.size(); k++)
          if (k != j) punct = mulmod(punct, B[k] % p, p);
        if (!run_floor_cases(p, invmod(qm, p), invmod(punct, p), rng, 40000)) return 1;
      }
    }
  }
  std::printf("ok %lld\n", g_total);
  return 0;
}
