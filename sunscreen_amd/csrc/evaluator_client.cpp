// sunscreen_amd/csrc/evaluator_client.cpp -- batched BatchEncoder / Decryptor / Encryptor on the device
// (the steps either side of the evaluator path; kernels in kernels_client.hip).
//
// Reference interfaces: seal_fhe/src/encoder.rs:75-190 (BatchEncoder_Encode1/2, Decode1/2),
// seal_fhe/src/encryptor_decryptor.rs:238-254 (Encryptor_Encrypt), :618-629 (Decryptor_Decrypt).
#include <algorithm>
#include <map>
#include <vector>

#include "evaluator.hpp"
#include "kernels.hpp"

namespace hipbfv {

namespace {
#define HC_CHECK(expr)                      \
  do {                                      \
    if ((expr) != hipSuccess) return kHipError; \
  } while (0)

#define HB_LAUNCH_CLIENT(id, units, expr)     \
  do {                                        \
    prof_.begin(id, units, s);                \
    hipError_t e__ = (expr);                  \
    prof_.end(s);                             \
    if (e__ != hipSuccess) return kHipError;  \
  } while (0)

NttPlan single_mod_plan(u32 m) {
  NttPlan pl{};
  pl.div = 1;
  pl.period = 1;
  pl.mod[0] = (unsigned char)m;
  return pl;
}
NttPlan range_plan(u32 count) {
  NttPlan pl{};
  pl.div = 1;
  pl.period = count;
  for (u32 i = 0; i < count; i++) pl.mod[i] = (unsigned char)i;
  return pl;
}
}  // namespace

// plain[op] = BatchEncoder_Encode(values[op]); values: u64[count][N] (or int64 when is_signed); *bad_host != 0 if a
// value lay outside the plain modulus (the plaintexts of such ops are not meaningful)
int Evaluator::batch_encode(const u64* values, u64* plain, size_t count, bool is_signed, u32* bad_host, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (!ctx_->batching()) return kUnsupported;
  ScratchGuard flag(pool_, sizeof(u32), s);
  if (!flag.p) return kOutOfMemory;
  HC_CHECK(hipMemsetAsync(flag.p, 0, sizeof(u32), s));
  const NttPlan plan = single_mod_plan(h.t_mod);
  for (size_t off = 0; off < count; off += 65535) {
    const size_t c = std::min<size_t>(65535, count - off);
    HC_CHECK(launch_batch_scatter(ctx_->dev(), h.n, ctx_->batch_index_map(), values + off * h.n, plain + off * h.n, c, is_signed ? 1 : 0, (u32*)flag.p, s));
    HC_CHECK(launch_ntt(ctx_->dev(), h.tw_inv, h.logn, plain + off * h.n, c, plan, true, 0, s));
  }
  u32 bad = 0;
  HC_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(u32), hipMemcpyDeviceToHost, s));
  HC_CHECK(hipStreamSynchronize(s));
  if (bad_host) *bad_host = bad;
  return kOk;
}

int Evaluator::batch_decode(const u64* plain, u64* values, size_t count, bool is_signed, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (!ctx_->batching()) return kUnsupported;
  const size_t chunk = std::min<size_t>(65535, std::max<size_t>(1, chunk_ops_ * 8));
  ScratchGuard tmp(pool_, std::min(chunk, count) * h.n * sizeof(u64), s);
  if (!tmp.p) return kOutOfMemory;
  const NttPlan plan = single_mod_plan(h.t_mod);
  for (size_t off = 0; off < count; off += chunk) {
    const size_t c = std::min(chunk, count - off);
    HC_CHECK(hipMemcpyAsync(tmp.p, plain + off * h.n, c * h.n * sizeof(u64), hipMemcpyDeviceToDevice, s));
    HC_CHECK(launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, (u64*)tmp.p, c, plan, false, 0, s));
    HC_CHECK(launch_batch_gather(ctx_->dev(), h.n, ctx_->batch_index_map(), (const u64*)tmp.p, values + off * h.n, c, is_signed ? 1 : 0, s));
  }
  return kOk;
}

// plain[op] = Decryptor_Decrypt(ct[op]) ; ct: u64[count][size][K][N], sk: u64[KK][N] in NTT form (SEAL SecretKey data).
// One phase computation c0 + c1*s + c2*s^2 ... per chunk feeds the plaintext rounding (plain != nullptr), the invariant-noise measure
// (noise != nullptr: NoiseOut) or both in one pass over the phase; at least one of the two outputs must be given.
int Evaluator::decrypt(const u64* ct, u32 size, const u64* sk_ntt, u64* plain, size_t count, hipStream_t s, const NoiseOut* noise) {
  const DevCtx& h = ctx_->host();
  if (size < 2 || !sk_ntt) return kInvalidArg;
  if (!plain && !(noise && noise->budget)) return kInvalidArg;
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, K = h.K;
  const size_t per = (size_t)(size - 1) * K;  // transformed residue polynomials per op
  const size_t chunk = std::max<size_t>(1, std::min<size_t>(chunk_ops_, 65535 / std::max<size_t>(per, 1)));
  const size_t cc = std::min(chunk, count);
  const size_t slab_words = noise ? (size_t)noise_blocks(n) * K : 0;  // per op: the noise measure's per-block maxima
  ScratchGuard sg(pool_, cc * ((per + K) * n + slab_words) * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* ctn = (u64*)sg.p;
  u64* acc = ctn + cc * per * n;
  u64* slab = acc + cc * K * n;
  const NttPlan plan = range_plan(K);
  const size_t cs = ctx_->ct_words(size);
  for (size_t off = 0; off < count; off += chunk) {
    const size_t c = std::min(chunk, count - off);
    // polys 1.. of every op, NTT'd: c_p (.) s^p accumulates in the transform domain
    HC_CHECK(hipMemcpy2DAsync(ctn, per * n * sizeof(u64), ct + off * cs + (size_t)K * n, cs * sizeof(u64), per * n * sizeof(u64), c,
                              hipMemcpyDeviceToDevice, s));
    HB_LAUNCH_CLIENT(kKernNttFwd, c * per, launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, ctn, c * per, plan, false, 0, s));
    if (size == 2 && h.logn <= 14) {  // c1 (.) s is formed while the inverse transform loads its input
      HB_LAUNCH_CLIENT(kKernNttInv, c * K, launch_ntt_inv_dyadic(ctx_->dev(), h.tw_inv, h.logn, ctn, sk_ntt, acc, K, 1, h.KK, c, s));
    } else {
      HC_CHECK(launch_dot_secret(ctx_->dev(), n, K, ctn, size, sk_ntt, acc, c, s));
      HB_LAUNCH_CLIENT(kKernNttInv, c * K, launch_ntt(ctx_->dev(), h.tw_inv, h.logn, acc, c * K, plan, true, 0, s));
    }
    u64* pl = plain ? plain + off * n : nullptr;
    if (!noise) {
      HC_CHECK(launch_decrypt_round(ctx_->dev(), n, ct + off * cs, size, acc, pl, c, s));
      continue;
    }
    HC_CHECK(launch_noise_partial(ctx_->dev(), ctx_->noise_consts(), n, K, ct + off * cs, size, acc, pl, slab, c, s));
    HC_CHECK(launch_noise_final(ctx_->noise_consts(), n, K, slab, noise->worst ? noise->worst + off * K : nullptr, noise->budget + off,
                                noise->noise ? noise->noise + off : nullptr, c, s));
  }
  return kOk;
}

// ---- KeyGenerator (seal_fhe/src/key_generator.rs:20-200; SEAL keygenerator.cpp) ----
// sk_coeff / sk_ntt: u64[KK][N] -- the ternary secret in coefficient form (kept for the Galois keys) and its transform
int Evaluator::keygen_secret(const RngSeed& seed, u64* sk_coeff, u64* sk_ntt, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  HC_CHECK(launch_keygen_ternary(ctx_->dev(), h.n, seed, 0, sk_coeff, s));
  HC_CHECK(hipMemcpyAsync(sk_ntt, sk_coeff, (size_t)h.KK * h.n * sizeof(u64), hipMemcpyDeviceToDevice, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, sk_ntt, h.KK, range_plan(h.KK), false, 0, s));
  return kOk;
}

// `count` key-level encryptions of zero under sk_ntt, the z-th one carrying w (.) (q_sp mod q_z) on residue z when w is
// given: count = 1, w = nullptr -> public key u64[2][KK][N]; count = K, w = s^2 or sigma_g(s) (NTT form) -> one
// key-switching key u64[K][2][KK][N].  `stream` keys the randomness (distinct per key).
int Evaluator::keygen_zero_encryptions(const RngSeed& seed, u64 stream, const u64* sk_ntt, const u64* w, u64* key, u32 count, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, KK = h.KK;
  ScratchGuard sg(pool_, (size_t)count * 2 * KK * n * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* a = (u64*)sg.p;
  u64* e = a + (size_t)count * KK * n;
  HC_CHECK(launch_keygen_sample(ctx_->dev(), n, seed, stream << 8, a, e, count, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, e, (size_t)count * KK, range_plan(KK), false, 0, s));
  HC_CHECK(launch_keygen_assemble(ctx_->dev(), n, KK, a, e, sk_ntt, w, key, count, s));
  return kOk;
}

// out[KK][N] = sigma_g(s) in coefficient form: the w of a Galois key before its transform
int Evaluator::keygen_galois_poly(const u64* sk_coeff, u32 galois_elt, u64* out, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  if (!(galois_elt & 1) || galois_elt >= 2 * h.n) return kInvalidArg;
  u64 inv = 1;
  for (int i = 0; i < 6; i++) inv = inv * (2 - (u64)galois_elt * inv);
  HC_CHECK(launch_keygen_galois(ctx_->dev(), h.n, h.KK, sk_coeff, out, (u32)(inv & (2 * h.n - 1)), s));
  return kOk;
}

// relin: w = s^2; galois element g: w = NTT(sigma_g(s)).  key: u64[K][2][KK][N]
int Evaluator::keygen_kswitch(const RngSeed& seed, u64 stream, const u64* sk_coeff, const u64* sk_ntt, u32 galois_elt, u64* key, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.KK < 2) return kNoKey;  // no special prime: SEAL refuses to create key-switching keys
  const u32 n = h.n, KK = h.KK;
  ScratchGuard sg(pool_, (size_t)KK * n * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* w = (u64*)sg.p;
  if (galois_elt == 0) {
    HC_CHECK(launch_keygen_square(ctx_->dev(), n, KK, sk_ntt, w, s));
  } else {
    if (int st = keygen_galois_poly(sk_coeff, galois_elt, w, s)) return st;
    HC_CHECK(launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, w, KK, range_plan(KK), false, 0, s));
  }
  return keygen_zero_encryptions(seed, stream, sk_ntt, w, key, h.K, s);
}

// ---- plaintext-matrix x ciphertext-vector products (the first loop nest of examples/pir/src/main.rs:16-45) ----
// pntt[op][K][N] = NTT(centred lift of plain[op]) -- what SEAL's multiply_plain computes internally for its plaintext
// operand (including the monomial rule, kernels.hip plain_lift_kernel).  A static database is transformed once.
int Evaluator::plain_to_ntt(const u64* plain, size_t pstride, u64* pntt, size_t count, hipStream_t s, int watch_zero) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, K = h.K;
  const size_t chunk = std::max<size_t>(1, 65535 / K);
  ScratchGuard nz(pool_, std::min(chunk, count) * sizeof(u32), s);
  if (!nz.p) return kOutOfMemory;
  const NttPlan plan = range_plan(K);
  for (size_t off = 0; off < count; off += chunk) {
    const size_t c = std::min(chunk, count - off);
    u64* out = pntt + off * (size_t)K * n;
    HC_CHECK(launch_plain_lift(ctx_->dev(), n, plain + off * pstride, pstride, out, c, (u32*)nz.p, s));
    if (watch_zero && watch_status()) HC_CHECK(launch_zero_plain_watch((const u32*)nz.p, watch_zero == 1 ? (u32)off : 0u, watch_zero == 1 ? 1u : 0u, (u32)c, watch_status(), s));
    HB_LAUNCH_CLIENT(kKernNttFwd, c * K, launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, out, c * K, plan, false, 0, s));
  }
  return kOk;
}

// ctn = NTT of every polynomial of ct (u64[count][size][K][N]); may be in place
int Evaluator::ct_to_ntt(const u64* ct, u32 size, u64* ctn, size_t count, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  const u32 K = h.K;
  const size_t polys = count * size * K;
  if (ctn != ct) HC_CHECK(hipMemcpyAsync(ctn, ct, polys * h.n * sizeof(u64), hipMemcpyDeviceToDevice, s));
  const NttPlan plan = range_plan(K);
  const size_t step = (65535 / K) * K;
  for (size_t off = 0; off < polys; off += step) {
    const size_t c = std::min(step, polys - off);
    HB_LAUNCH_CLIENT(kKernNttFwd, c, launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, ctn + off * h.n, c, plan, false, 0, s));
  }
  return kOk;
}

// out[row] = sum_j multiply_plain(ct_j, plain[row][j]) for size-2 ciphertexts, from the transformed operands:
// ctn: u64[cols][2][K][N] (ct_to_ntt), pntt: u64[rows][cols][K][N] (plain_to_ntt), out: u64[rows][2][K][N] coefficient form.
// Bit-identical to SEAL's sequence of multiply_plain and add (every step there is exact modular arithmetic).
int Evaluator::dot_plain_ntt(const u64* ctn, u32 cols, const u64* pntt, u32 rows, u64* out, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  if (!cols || !rows) return kInvalidArg;
  const u32 n = h.n, K = h.K;
  const NttPlan plan = range_plan(K);
  const u32 step = 65535 / (2 * K) / 8 * 8;  // rows per launch: the inverse transform covers rows * 2 * K polynomials
  for (u32 off = 0; off < rows; off += step) {
    const u32 c = std::min(step, rows - off);
    u64* o = out + (size_t)off * 2 * K * n;
    HB_LAUNCH_CLIENT(kKernPlain, (size_t)c * cols, launch_dot_plain(ctx_->dev(), n, K, ctn, cols, pntt + (size_t)off * cols * K * n, c, o, s));
    HB_LAUNCH_CLIENT(kKernNttInv, (size_t)c * 2 * K, launch_ntt(ctx_->dev(), h.tw_inv, h.logn, o, (size_t)c * 2 * K, plan, true, 0, s));
  }
  return kOk;
}

DotQueriesTile dot_queries_tile() {
  if (const char* env = std::getenv("HIPBFV_DOT_QUERIES_TILE")) {
    char* end = nullptr;
    const unsigned long rt = std::strtoul(env, &end, 10);
    const unsigned long qt = end && *end == 'x' ? std::strtoul(end + 1, nullptr, 10) : 0;
    for (const DotQueriesTile& t : kDotQueriesTiles)
      if (t.RT == rt && t.QT == qt) return t;
  }
  return kDotQueriesTiles[0];
}

// Many queries, one pass over the database (dot_plain_q_kernel: each database word multiplied in registers against a tile of
// queries).  out[q] is dot_plain_ntt's result for query q, bit for bit: the same exact modular sums in another order.
int Evaluator::dot_plain_ntt_queries(const u64* ctn, u32 queries, u32 cols, const u64* pntt, u32 rows, u64* out, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  if (!cols || !rows) return kInvalidArg;
  if (!queries) return kOk;
  const u32 n = h.n, K = h.K;
  const size_t ctw = (size_t)2 * K * n;
  if (int rc = plan_dot_queries(queries, rows, K, dot_queries_tile(), [&](const DotQueriesStep& st) -> int {
        const u64* c = ctn + (size_t)st.query0 * cols * ctw;
        u64* o = out + (size_t)st.query0 * rows * ctw;
        if (st.QT == 1)
          HB_LAUNCH_CLIENT(kKernPlain, (size_t)rows * cols, launch_dot_plain(ctx_->dev(), n, K, c, cols, pntt, rows, o, s));
        else
          HB_LAUNCH_CLIENT(kKernPlain, (size_t)st.queries * rows * cols,
                           launch_dot_plain_queries(ctx_->dev(), n, K, c, (u32)st.queries, cols, pntt, rows, o, st.RT, st.QT, s));
        return kOk;
      }))
    return rc;
  const NttPlan plan = range_plan(K);
  const size_t polys = (size_t)queries * rows * 2 * K, step = (65535 / K) * K;
  for (size_t off = 0; off < polys; off += step) {
    const size_t c = std::min(step, polys - off);
    HB_LAUNCH_CLIENT(kKernNttInv, c, launch_ntt(ctx_->dev(), h.tw_inv, h.logn, out + off * n, c, plan, true, 0, s));
  }
  return kOk;
}

// The graph executor's matrix-vector product (program_plan.cpp): as dot_plain_ntt with the plaintexts behind a descriptor table
// and a batch dimension.
int Evaluator::dot_plain_tab(const u64* ctn, u32 cols, const PlainNttRef* tab, u32 rows, u32 batch, u64* out, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  if (!cols || !rows || !batch) return kInvalidArg;
  const u32 n = h.n, K = h.K;
  const NttPlan plan = range_plan(K);
  HB_LAUNCH_CLIENT(kKernPlain, (size_t)rows * cols * batch, launch_dot_plain_tab(ctx_->dev(), n, K, ctn, cols, tab, rows, batch, out, s));
  const size_t polys = (size_t)rows * batch * 2 * K, step = (65535 / K) * K;
  for (size_t off = 0; off < polys; off += step) {
    const size_t c = std::min(step, polys - off);
    HB_LAUNCH_CLIENT(kKernNttInv, c, launch_ntt(ctx_->dev(), h.tw_inv, h.logn, out + off * n, c, plan, true, 0, s));
  }
  return kOk;
}

int Evaluator::multiply_plain_ntt(const u64* ct, u32 size, const u64* pntt, size_t pnstride, u64* out, size_t count, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (size < 2 || !pntt) return kInvalidArg;
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, K = h.K;
  if (int rc = ct_to_ntt(ct, size, out, count, s)) return rc;
  const NttPlan plan = range_plan(K);
  const size_t cs = ctx_->ct_words(size);
  for (size_t off = 0; off < count; off += 65535) {
    const size_t c = std::min<size_t>(65535, count - off);
    HC_CHECK(launch_dyadic_plain(ctx_->dev(), n, K, out + off * cs, size, pntt + off * pnstride, pnstride, c, s));
  }
  const size_t polys = count * size * K, step = (65535 / K) * K;
  for (size_t off = 0; off < polys; off += step) {
    const size_t c = std::min(step, polys - off);
    HB_LAUNCH_CLIENT(kKernNttInv, c, launch_ntt(ctx_->dev(), h.tw_inv, h.logn, out + off * n, c, plan, true, 0, s));
  }
  return note_result(out, size, K, count, s);
}

int Evaluator::note_nary(const NaryOut* douts, u32 nouts, u32 batch, hipStream_t s) {
  u32* status = watch_status();
  if (!status || !nouts) return kOk;
  HC_CHECK(launch_transparent_watch_nary(ctx_->dev(), douts, nouts, batch, status, s));
  return kOk;
}

// ct2[op] = Encryptor_Encrypt(plain[op]) under the public key pk: u64[2][KK][N] (NTT form, key level).
// Randomness: ChaCha20 blocks keyed by `seed.secret` (rng.hpp), counter = (coefficient, first_op + op): reproducible and independent of
// the chunking.  plain: u64[count][N] (pstride = N) or one shared plaintext (pstride = 0).
int Evaluator::encrypt(const u64* plain, size_t pstride, const u64* pk, const RngSeed& seed, u64 first_op, u64* ct2, size_t count, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (!pk) return kInvalidArg;
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, K = h.K, KK = h.KK;
  const size_t chunk = std::max<size_t>(1, std::min<size_t>(chunk_ops_, 65535 / (2 * (size_t)KK)));
  const size_t cc = std::min(chunk, count);
  // u[KK] + c[2][KK] residue polynomials per op; the error polynomials are regenerated where they are consumed
  ScratchGuard sg(pool_, cc * 3 * (size_t)KK * n * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* u = (u64*)sg.p;
  u64* c2 = u + cc * (size_t)KK * n;
  const NttPlan plan = range_plan(KK);
  for (size_t off = 0; off < count; off += chunk) {
    const size_t c = std::min(chunk, count - off);
    HC_CHECK(launch_encrypt_sample(ctx_->dev(), n, seed, first_op + off, u, nullptr, c, s));
    HB_LAUNCH_CLIENT(kKernNttFwd, c * KK, launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, u, c * KK, plan, false, 0, s));
    if (h.logn <= 14) {  // pk (.) NTT(u) is formed while the inverse transform loads its input
      HB_LAUNCH_CLIENT(kKernNttInv, c * 2 * KK, launch_ntt_inv_dyadic(ctx_->dev(), h.tw_inv, h.logn, u, pk, c2, KK, 2, KK, c, s));
    } else {
      HC_CHECK(launch_encrypt_dyadic(ctx_->dev(), n, KK, u, pk, c2, c, s));
      HB_LAUNCH_CLIENT(kKernNttInv, c * 2 * KK, launch_ntt(ctx_->dev(), h.tw_inv, h.logn, c2, c * 2 * KK, plan, true, 0, s));
    }
    // + e, SEAL's divide-and-round by the special prime (the mod_switch of the fresh key-level encryption) and
    // + round(q/t * m) with SEAL's rounding correction (multiply_add_plain_with_scaling_variant), in one pass
    HC_CHECK(launch_encrypt_finish(ctx_->dev(), n, seed, first_op + off, c2, plain + off * pstride, pstride, ct2 + off * 2 * K * n, c, s));
  }
  return kOk;
}

// First K residue rows of each of `polys` key-level polynomials: src u64[polys][KK][N] -> dst u64[polys][K][N]
static hipError_t take_data_rows(const DevCtx& h, const u64* src, u64* dst, u32 polys, hipStream_t s) {
  const size_t row = (size_t)h.n * sizeof(u64);
  return hipMemcpy2DAsync(dst, h.K * row, src, h.KK * row, h.K * row, polys, hipMemcpyDeviceToDevice, s);
}

// One public-key encryption that also hands back what was sampled (the fork's Encryptor_EncryptReturnComponents,
// seal_fhe/src/encryptor_decryptor.rs:268-300): u_out u64[K][N] (ternary), e_out u64[2][K][N], coefficient-form data-level
// residues.  no_special: compute (pk*u + e) on the data primes only, with no division by the special prime, so that
// c0 = floor(q/t)*m + r + pk0*u + e0 and c1 = pk1*u + e1 hold EXACTLY (what logproof proves, bfv_statement.rs:159).
int Evaluator::encrypt_components(const u64* plain, const u64* pk, const RngSeed& seed, u64 op, bool no_special, u64* ct2, u64* u_out, u64* e_out,
                                  hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (!pk) return kInvalidArg;
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, KK = h.KK;
  ScratchGuard sg(pool_, 5 * (size_t)KK * n * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* u = (u64*)sg.p;
  u64* e = u + (size_t)KK * n;
  u64* c2 = e + 2 * (size_t)KK * n;
  const NttPlan plan = range_plan(KK);
  HC_CHECK(launch_encrypt_sample(ctx_->dev(), n, seed, op, u, e, 1, s));
  if (u_out) HC_CHECK(take_data_rows(h, u, u_out, 1, s));
  if (e_out) HC_CHECK(take_data_rows(h, e, e_out, 2, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, u, KK, plan, false, 0, s));
  HC_CHECK(launch_encrypt_dyadic(ctx_->dev(), n, KK, u, pk, c2, 1, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_inv, h.logn, c2, 2 * KK, plan, true, 0, s));
  HC_CHECK(launch_add_key_level(ctx_->dev(), n, c2, e, 2 * KK, s));
  if (KK > 1 && !no_special) {
    HC_CHECK(launch_ks_moddown(ctx_->dev(), n, c2, nullptr, 0, 0u, nullptr, ct2, 1, s));
  } else {
    HC_CHECK(take_data_rows(h, c2, ct2, 2, s));
  }
  return add_plain(ct2, 2, plain, 0, ct2, 1, s);
}

// Secret-key encryption (SEAL encrypt_zero_symmetric at the data level + scaled plaintext): c1 = a uniform,
// c0 = floor(q/t)*m + r - (a*s + e).  e_out (optional): u64[K][N] coefficient-form residues of e.
int Evaluator::encrypt_symmetric(const u64* plain, const u64* sk_ntt, const RngSeed& seed, u64 stream, u64* ct2, u64* e_out, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (!sk_ntt) return kInvalidArg;
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, KK = h.KK;
  ScratchGuard sg(pool_, 4 * (size_t)KK * n * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* a = (u64*)sg.p;
  u64* e = a + (size_t)KK * n;
  u64* c = e + (size_t)KK * n;
  const NttPlan plan = range_plan(KK);
  HC_CHECK(launch_keygen_sample(ctx_->dev(), n, seed, stream << 8, a, e, 1, s));
  if (e_out) HC_CHECK(take_data_rows(h, e, e_out, 1, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_fwd, h.logn, e, KK, plan, false, 0, s));
  HC_CHECK(launch_keygen_assemble(ctx_->dev(), n, KK, a, e, sk_ntt, nullptr, c, 1, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_inv, h.logn, c, 2 * KK, plan, true, 0, s));
  HC_CHECK(take_data_rows(h, c, ct2, 2, s));
  return add_plain(ct2, 2, plain, 0, ct2, 1, s);
}

// Key-level NTT-form polynomials (public / secret key) as data-level coefficient-form residues: u64[polys][K][N]
int Evaluator::key_to_coeff(const u64* key, u32 polys, u64* out, hipStream_t s) {
  const DevCtx& h = ctx_->host();
  if (h.logn > 15) return kUnsupported;
  const u32 n = h.n, KK = h.KK;
  ScratchGuard sg(pool_, (size_t)polys * KK * n * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* tmp = (u64*)sg.p;
  HC_CHECK(hipMemcpyAsync(tmp, key, (size_t)polys * KK * n * sizeof(u64), hipMemcpyDeviceToDevice, s));
  HC_CHECK(launch_ntt(ctx_->dev(), h.tw_inv, h.logn, tmp, (size_t)polys * KK, range_plan(KK), true, 0, s));
  HC_CHECK(take_data_rows(h, tmp, out, polys, s));
  return kOk;
}

int Evaluator::crt_compose(const u64* consts, u32 kc, const u64* in, u64* out, u32 polys, hipStream_t s) {
  HC_CHECK(launch_crt_compose(ctx_->dev(), ctx_->host().n, kc, consts, in, out, polys, s));
  return kOk;
}
int Evaluator::crt_decompose(u32 kc, const u64* in, u64* out, u32 polys, hipStream_t s) {
  HC_CHECK(launch_crt_decompose(ctx_->dev(), ctx_->host().n, kc, in, out, polys, s));
  return kOk;
}

// g^{-1} mod 2n (Newton iteration, g odd)
static u32 galois_inverse_of(u32 elt, u32 n) {
  u64 inv = 1;
  for (int i = 0; i < 6; i++) inv = inv * (2 - (u64)elt * inv);
  return (u32)(inv & (2 * n - 1));
}

// tables of item addresses in pinned memory the device reads directly; back to the pool behind the stream's last launch
namespace {
struct PinnedTables {
  PinnedPool& pool;
  hipStream_t s;
  void* p;
  ~PinnedTables() {
    if (p) pool.release(p, s);
  }
};
}  // namespace

// ---- mixed-step rotation batches with one key set per client (kept apart from evaluator.cpp's single-set apply_galois_items, whose
// callers and launch sequences stay as they are) ----
// Item i by its own element elts[i] through its own key keys[i].  Where apply_galois would read the automorphism through the key
// switch, ONE head / middle / tail sequence per chunk serves every element and every client: the head and the tail take item i's g^-1
// from a device table (kernels_split.hip GinvArg), the middle kernel takes item i's key through the KeyMap -- one entry of the key table
// per distinct (key, element) pair, the walk sorted by (element, key), so that the items that share a key share its rows in an XCD's L2
// as the items of one client do.  Copied and left-out items stay in the grid (their workgroups leave at once): the chunk keeps the
// caller's item numbering, no gather.  Elsewhere (in place, the whole-polynomial kernels, N outside 4096 ... 16384,
// HIPBFV_NO_FUSED_GALOIS) the items are grouped by (key, element) and every group goes through apply_galois on a compact stage; the
// bits are the same.  key_ids (optional): the caller's number of item i's key set -- the order of the keys of one element in the
// table (without it: the order in which the key pointers first appear).
int Evaluator::apply_galois_items_keyed(const u64* ct2, const u32* elts, const u64* const* keys, const u32* key_ids, u64* out2, size_t count, hipStream_t s,
                                        bool watch) {
  const DevCtx& h = ctx_->host();
  const u32 n = h.n, K = h.K;
  if (!count) return kOk;
  if (!elts) return kInvalidArg;
  // distinct (element > 1, key) pairs; kidx[i]: item i's entry, kKeyNone for a copied or left-out item
  std::vector<u32> delt, kidx(count, kKeyNone);
  std::vector<const u64*> dkey;
  {
    std::map<const u64*, u32> seen_key;                // key pointer -> id, where the caller numbers no sets
    std::map<std::pair<u32, u32>, u32> entry_of;      // (element, key id) -> entry: the map's order is the walk's
    std::vector<std::pair<u32, u32>> pair_of(count);
    for (size_t i = 0; i < count; i++) {
      const u32 e = elts[i];
      if (e <= 1) continue;
      if (!(e & 1) || e >= 2 * n) return kInvalidArg;
      if (h.KK < 2 || !keys || !keys[i]) return kNoKey;
      const u32 id = key_ids ? key_ids[i] : seen_key.emplace(keys[i], (u32)seen_key.size()).first->second;
      pair_of[i] = {e, id};
      entry_of.emplace(pair_of[i], 0u);
    }
    delt.resize(entry_of.size());
    dkey.assign(entry_of.size(), nullptr);
    u32 d = 0;
    for (auto& kv : entry_of) kv.second = d++;
    for (size_t i = 0; i < count; i++) {
      if (elts[i] <= 1) continue;
      const u32 at = entry_of[pair_of[i]];
      kidx[i] = at;
      delt[at] = elts[i];
      if (!dkey[at]) dkey[at] = keys[i];
      if (dkey[at] != keys[i]) return kInvalidArg;  // one key id, two keys
    }
  }
  if (h.logn > 15) return kUnsupported;
  const size_t rot_words = (size_t)2 * K * n;
  if (ct2 != out2) {  // element 1: runs of neighbouring items, one copy each
    for (size_t i = 0; i < count;) {
      size_t r = 0;
      while (i + r < count && elts[i + r] == 1) r++;
      if (r) HC_CHECK(launch_copy_words(ct2 + i * rot_words, out2 + i * rot_words, r * rot_words, s));
      i += r ? r : 1;
    }
  }
  if (delt.empty()) return watch ? note_result(out2, 2, K, count, s) : (int)kOk;
  const size_t chunk = std::max<size_t>(1, std::min<size_t>(chunk_ops_, 65535 / ((size_t)h.KK * K)));
  const size_t cc = std::min(chunk, count);
  const size_t last = count % chunk ? count % chunk : cc;
  const bool fused = fuse_galois_ && ct2 != out2 && h.logn >= 12 && h.logn <= 14 && ks_split_for(cc) && ks_split_for(last);
  if (fused) {
    std::vector<u32> ginv(count);
    for (size_t i = 0; i < count; i++) ginv[i] = kidx[i] == kKeyNone ? kGinvSkip : galois_inverse_of(elts[i], n);
    KeySel sel;
    sel.keys = dkey.data();
    sel.nkeys = (u32)dkey.size();
    sel.index = kidx.data();
    sel.period = count;
    KeyMapLease kl;
    if (int rc = stage_keymap(sel, count, chunk, s, kl, ginv.data())) return rc;
    ScratchGuard sg(pool_, cc * ks_scratch_words() * sizeof(u64), s);
    if (!sg.p) return kOutOfMemory;
    for (size_t off = 0; off < count; off += chunk) {
      const size_t c = std::min(chunk, count - off);
      if (std::all_of(kidx.begin() + off, kidx.begin() + off + c, [](u32 k) { return k == kKeyNone; })) continue;
      const u64* in = ct2 + off * rot_words;
      int rc = key_switch(in + (size_t)K * n, rot_words, nullptr, in, rot_words, 1u, out2 + off * rot_words, c, (u64*)sg.p, s, nullptr, kl.at(off), 0, kl.words + off);
      if (rc) return rc;
    }
    return watch ? note_result(out2, 2, K, count, s) : (int)kOk;
  }
  // grouped: per (key, element) pair, the group's items gathered into a compact stage, rotated by the uniform path, scattered to their places
  // (a group that is the whole call needs no stage).  The tables of item addresses live in pinned memory the device reads directly.
  {
    WatchScope quiet(nullptr);  // the groups' own item numbers mean nothing to the caller: the results are noted once, below
    if (delt.size() == 1 && std::all_of(kidx.begin(), kidx.end(), [](u32 k) { return k == 0; })) {
      if (int rc = apply_galois(ct2, delt[0], dkey[0], out2, count, s)) return rc;
    } else {
      const size_t sub = std::min<size_t>(chunk_ops_, 32768);  // items per stage (and per gather / scatter grid)
      PinnedTables tabs{pinned_, s, pinned_.acquire(2 * count * sizeof(u64*))};
      if (!tabs.p) return kOutOfMemory;
      const u64** src = static_cast<const u64**>(tabs.p);
      u64** dst = static_cast<u64**>(tabs.p) + count;
      size_t filled = 0, largest = 0;
      std::vector<size_t> first(delt.size() + 1, 0);
      for (size_t d = 0; d < delt.size(); d++) {
        for (size_t i = 0; i < count; i++)
          if (kidx[i] == d) src[filled] = ct2 + i * rot_words, dst[filled] = out2 + i * rot_words, filled++;
        first[d + 1] = filled;
        largest = std::max(largest, std::min(sub, filled - first[d]));
      }
      ScratchGuard sg(pool_, 2 * largest * rot_words * sizeof(u64), s);
      if (!sg.p) return kOutOfMemory;
      u64* in_stage = (u64*)sg.p;
      u64* out_stage = in_stage + largest * rot_words;
      for (size_t d = 0; d < delt.size(); d++) {
        for (size_t off = first[d]; off < first[d + 1]; off += sub) {
          const size_t c = std::min(sub, first[d + 1] - off);
          HC_CHECK(launch_gather_items(src + off, in_stage, rot_words, c, s));
          if (int rc = apply_galois(in_stage, delt[d], dkey[d], out_stage, c, s)) return rc;
          HC_CHECK(launch_scatter_items(out_stage, dst + off, rot_words, c, s));
        }
      }
    }
  }
  return watch ? note_result(out2, 2, K, count, s) : (int)kOk;
}

// NAF chains in shared rounds (mixed-step rotation batches with one key set per client): batch item items[j] goes through the
// elements elts[r * nitems + j], r = 0 ... (0 from the round on in which it has finished), each through keys[r * nitems + j].  The
// items are gathered ONCE into a compact stage with a twin; round r is ONE apply_galois_items_keyed call from one stage into the other
// (out of place: the fused launch sequence serves it; finished items are left out), whatever the steps and the clients; every item
// is scattered from the stage it finished in.  The stage lists the items that finish in the first stage (an even number of
// rounds) ahead of the others, so that two scatter launches do.  The results are not noted: the caller does, once all are in place.
int Evaluator::apply_galois_rounds(const u64* ct2, u64* out2, const u64* items, size_t nitems, u32 rounds, const u32* elts, const u64* const* keys,
                                   const u32* key_ids, hipStream_t s) {
  if (!nitems || !rounds) return kOk;
  if (!items || !elts || !keys) return kInvalidArg;
  const DevCtx& h = ctx_->host();
  const size_t w = (size_t)2 * h.K * h.n;
  const size_t sub = std::min<size_t>(chunk_ops_, 32768);  // items per stage (and per gather / scatter grid)
  const size_t cc = std::min(sub, nitems);
  PinnedTables tabs{pinned_, s, pinned_.acquire(2 * nitems * sizeof(u64*))};
  if (!tabs.p) return kOutOfMemory;
  const u64** src = static_cast<const u64**>(tabs.p);
  u64** dst = static_cast<u64**>(tabs.p) + nitems;
  ScratchGuard sg(pool_, 2 * cc * w * sizeof(u64), s);
  if (!sg.p) return kOutOfMemory;
  u64* const stage[2] = {(u64*)sg.p, (u64*)sg.p + cc * w};
  WatchScope quiet(nullptr);
  std::vector<u32> len(nitems), e, ids;
  std::vector<size_t> order;
  std::vector<const u64*> k;
  for (size_t j = 0; j < nitems; j++)
    while (len[j] < rounds && elts[(size_t)len[j] * nitems + j]) len[j]++;
  for (size_t b = 0; b < nitems; b += sub) {
    const size_t c = std::min(sub, nitems - b);
    order.clear();
    u32 longest = 0;
    for (u32 parity = 0; parity < 2; parity++)
      for (size_t j = b; j < b + c; j++)
        if ((len[j] & 1u) == parity) order.push_back(j);
    const size_t first_stage = std::count_if(order.begin(), order.end(), [&](size_t j) { return !(len[j] & 1u); });
    for (size_t p = 0; p < c; p++) {
      src[b + p] = ct2 + items[order[p]] * w;
      dst[b + p] = out2 + items[order[p]] * w;
      longest = std::max(longest, len[order[p]]);
    }
    HC_CHECK(launch_gather_items(src + b, stage[0], w, c, s));
    e.resize(c), ids.resize(c), k.resize(c);
    for (u32 r = 0; r < longest; r++) {
      for (size_t p = 0; p < c; p++) {
        const size_t at = (size_t)r * nitems + order[p];
        e[p] = r < len[order[p]] ? elts[at] : 0u;
        k[p] = keys[at];
        ids[p] = key_ids ? key_ids[order[p]] : 0u;
      }
      if (int rc = apply_galois_items_keyed(stage[r & 1], e.data(), k.data(), key_ids ? ids.data() : nullptr, stage[(r + 1) & 1], c, s, false)) return rc;
    }
    if (first_stage) HC_CHECK(launch_scatter_items(stage[0], dst + b, w, first_stage, s));
    if (c - first_stage) HC_CHECK(launch_scatter_items(stage[1] + first_stage * w, dst + b + first_stage, w, c - first_stage, s));
  }
  return kOk;
}

}  // namespace hipbfv
