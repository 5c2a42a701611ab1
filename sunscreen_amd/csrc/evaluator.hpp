// sunscreen_amd/csrc/evaluator.hpp -- the GPU batch executor for the Evaluator operations.
//
// Mirrors the operation set of `trait seal_fhe::Evaluator` (seal_fhe/src/evaluator.rs:7-280) with an
// extra leading batch dimension that the reference does not have: every method processes `count`
// independent ciphertexts laid out contiguously in HBM (u64[count][size][K][N]) with one sequence of
// kernel launches, instead of one FFI call per graph node (sunscreen_runtime/src/run.rs:160-341).
// All pointers are device pointers; all work is enqueued on the given HIP stream and is asynchronous.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "context.hpp"
#include "kernels.hpp"

namespace hipbfv {

enum Status : int {
  kOk = 0,
  kInvalidArg = -1,
  kTransparent = -2,
  kNoKey = -3,
  kOutOfMemory = -4,
  kHipError = -5,
  kUnsupported = -6,
};

// Stream-aware caching allocator for kernel scratch space.
class ScratchPool {
 public:
  ~ScratchPool();
  void* acquire(size_t bytes, hipStream_t s);
  void release(void* p, hipStream_t s);
  void trim();

 private:
  struct Block {
    void* ptr;
    size_t bytes;
    hipStream_t last;
    hipEvent_t ev;
    bool busy;
  };
  std::mutex mu_;
  std::vector<Block> blocks_;
};

// Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline figures).
enum KernelId : int {
  kKernNttFwd = 0,
  kKernNttInv,
  kKernBehzExtend,
  kKernTensor,
  kKernBehzFloorSk,
  kKernKsDecompose,
  kKernKsMac,
  kKernKsModdown,
  kKernGalois,
  kKernEltwise,
  kKernPlain,
  kKernKsHead,
  kKernKsMid,
  kKernKsTail,
  kKernKsTailSum,  // the summing tail of rotate_sum; kinds are read by name, so it sits beside its twin
  kKernMulHead,
  kKernMulMid,
  kKernMulPrep,  // the forward half alone (prepared multiplicands); kinds are read by name, so it sits beside its twin
  kKernMulTail,
  kKernMulTailSum,
  kKernCount
};
const char* kernel_name(int id);

class Profiler {
 public:
  ~Profiler();
  bool enabled = false;
  // record the start/stop events around one launch; `units` = work items of that launch (e.g. residue polys)
  void begin(int id, size_t units, hipStream_t s);
  void end(hipStream_t s);
  // synchronise, accumulate finished records into the totals and recycle their events
  void collect();
  void reset();
  double total_ms[kKernCount] = {};
  unsigned long long launches[kKernCount] = {};
  unsigned long long units[kKernCount] = {};

 private:
  struct Rec {
    int id;
    size_t units;
    hipEvent_t a, b;
  };
  std::mutex mu_;
  std::vector<Rec> recs_;
  std::vector<hipEvent_t> free_;
  hipEvent_t get_event();
};

// Pinned host staging blocks for small tables that a launch sequence reads after the call has returned (the per-item key maps).
// Like ScratchPool, but a block is handed out again only after the copy out of it has finished (the HOST overwrites it).
class PinnedPool {
 public:
  ~PinnedPool();
  void* acquire(size_t bytes);
  void release(void* p, hipStream_t s);  // the copies out of the block were enqueued on `s`

 private:
  struct Block {
    void* ptr;
    size_t bytes;
    hipEvent_t ev;
    bool busy, pending;
  };
  std::mutex mu_;
  std::vector<Block> blocks_;
};

// Which key-switching key each item of a batch uses.  The reference hands the keys over with every call
// (sunscreen_runtime/src/run.rs:100-105: `relin_keys: &Option<&RelinearizationKeys>`, `galois_keys`; runtime.rs:310-327), so a
// server that batches the calls of many clients holds one key set per client: item i of the batch uses
// keys[index[(first + i) % period]] (period = the number of input sets: the graph executor's merged launches number their
// ciphertexts member-major, item = member * period + set).  keys == nullptr: the one key `key` for every item.
struct KeySel {
  const u64* key = nullptr;          // device, u64[K][2][K+1][N]
  const u64* const* keys = nullptr;  // HOST array of nkeys device pointers
  u32 nkeys = 0;
  const u32* index = nullptr;        // HOST array of `period` key indices
  size_t period = 0;
  size_t first = 0;                  // the batch's item 0 is item `first` of the selection
  KeySel() = default;
  KeySel(const u64* one) : key(one) {}  // NOLINT: every single-key call site passes its pointer
  bool per_item() const { return keys != nullptr; }
  bool present() const { return per_item() ? nkeys != 0 : key != nullptr; }
};

// A prepared multiplicand (Evaluator::prepare_multiplicand): `count` ciphertexts kept for products that share their second operand.
//  ct   = a copy of the canonical ciphertexts, u64[count][2][K][N] (the paths that run the whole-polynomial kernels gather from it);
//  rows = both polynomials of every ciphertext extended to all R = K + S residues and forward-transformed, u64[count][2][R][N], as the
//         middle kernel holds them in front of the tensor product (kernels.hpp launch_mul_prep_mid) -- nullptr where the parameter
//         set has no split multiply.
// ready is recorded behind the last launch that fills the buffers; every call that uses the object makes its stream wait on it.
struct Multiplicand {
  Context* ctx = nullptr;
  u64* ct = nullptr;
  u64* rows = nullptr;
  size_t count = 0;
  size_t bytes = 0;
  hipEvent_t ready = nullptr;
  ~Multiplicand();
};

// Which prepared ciphertext each item of a *_shared call multiplies by: item i by m->ct[index[(first + i) % period]] (index: a HOST
// array, every entry below m->count -- the callers check).
struct SharedSel {
  const Multiplicand* m = nullptr;
  const u32* index = nullptr;
  size_t period = 0;
  size_t first = 0;
  SharedSel at(size_t off) const {
    SharedSel r = *this;
    r.first += off;
    return r;
  }
};

// Which two prepared ciphertexts each item of a *_prepared call multiplies: item i is ma->ct[a_index[(first + i) % period]] times
// mb->ct[b_index[(first + i) % period]] (HOST arrays, every entry below its object's count -- the callers check; ma may be mb).
struct PairSel {
  const Multiplicand* ma = nullptr;
  const Multiplicand* mb = nullptr;
  const u32* a_index = nullptr;
  const u32* b_index = nullptr;
  size_t period = 0;
  size_t first = 0;
  bool rows() const { return ma->rows && mb->rows; }
  PairSel at(size_t off) const {
    PairSel r = *this;
    r.first += off;
    return r;
  }
};

// The invariant-noise outputs of Evaluator::decrypt (device memory, one entry per item): budget = SEAL's invariant_noise_budget,
// noise (optional) = the fork's invariant_noise as a double, worst (optional) = u64[count][K] limbs of max_x |[t * phase(x)]_q|.
struct NoiseOut {
  int* budget = nullptr;
  double* noise = nullptr;
  u64* worst = nullptr;
};

// RAII lease of a scratch-pool buffer on a stream
struct ScratchGuard {
  ScratchPool& pool;
  hipStream_t s;
  void* p;
  ScratchGuard(ScratchPool& pl, size_t bytes, hipStream_t st) : pool(pl), s(st), p(pl.acquire(bytes, st)) {}
  ~ScratchGuard() {
    if (p) pool.release(p, s);
  }
  ScratchGuard(const ScratchGuard&) = delete;
  ScratchGuard& operator=(const ScratchGuard&) = delete;
};

// The launch sequences of Evaluator::multiply_sum (sums of `terms` products per group, `chunk` items of scratch), decided on the host:
// step = items [term0, term0 + terms) of the groups [group0, group0 + groups), multiplied together and summed by one launch.
//  - a chunk is a whole number of groups, max(1, chunk / terms) of them and at most 65535 (the groups are on grid z);
//  - a group with more terms than a chunk holds runs alone, in slices of `chunk` terms: the first slice writes the group's sums,
//    the later ones add onto them (accumulate).
struct MulSumStep {
  size_t group0, groups, term0, terms;
  bool accumulate;
};
template <class Visit>
int plan_multiply_sum(size_t groups, size_t terms, size_t chunk, Visit&& visit) {
  if (!terms || !chunk) return kInvalidArg;
  if (terms <= chunk) {
    const size_t per = std::min<size_t>(chunk / terms, 65535);
    for (size_t g = 0; g < groups; g += per)
      if (int rc = visit(MulSumStep{g, std::min(per, groups - g), 0, terms, false})) return rc;
    return 0;
  }
  for (size_t g = 0; g < groups; g++)
    for (size_t t0 = 0; t0 < terms; t0 += chunk)
      if (int rc = visit(MulSumStep{g, 1, t0, std::min(chunk, terms - t0), t0 != 0})) return rc;
  return 0;
}

// The product launches of Evaluator::dot_plain_ntt_queries (Q queries against one transformed database), decided on the host:
// step = the queries [query0, query0 + queries) against the rows [row0, row0 + rows) in ONE launch of dot_plain_q_kernel<RT, QT>, or,
// where QT == 1, of the single-query dot_plain2_kernel<RT>.
//  - one query runs the single-query kernel (kDotPlainRT rows per thread);
//  - otherwise the tile is `tile` (dot_queries_tile()) and the queries go in order, as many per launch as keep
//    ceil(rows / RT) * ceil(queries / QT) workgroups on grid x (2^31 - 1): a whole number of tiles, all queries in practice;
//  - a last launch left with a single query runs the single-query kernel.
// Every launch covers all rows.  K is validated only: today's rule does not depend on the number of residues.
struct DotQueriesTile {
  u32 RT, QT;
};
constexpr u32 kDotPlainRT = 4;  // launch_dot_plain's rows per thread
constexpr DotQueriesTile kDotQueriesTiles[] = {{2, 2}, {1, 4}, {1, 2}};  // the instantiations; the first is the default
// the tile in use: kDotQueriesTiles[0], or the one HIPBFV_DOT_QUERIES_TILE="<RT>x<QT>" names (tools/dot_plain_queries_timing.py)
DotQueriesTile dot_queries_tile();
struct DotQueriesStep {
  u64 query0, queries, row0, rows;
  u32 QT, RT;
};
template <class Visit>
int plan_dot_queries(u64 queries, u64 rows, u64 K, DotQueriesTile tile, Visit&& visit) {
  if (!rows || !K || queries > 0xFFFFFFFFull || rows > 0xFFFFFFFFull) return kInvalidArg;
  if (queries == 1) return visit(DotQueriesStep{0, 1, 0, rows, 1, kDotPlainRT});
  const u64 rowblocks = (rows + tile.RT - 1) / tile.RT;
  const u64 per = std::max<u64>(1, 0x7FFFFFFFull / rowblocks) * tile.QT;
  for (u64 q = 0; q < queries; q += per) {
    const u64 c = std::min(per, queries - q);
    if (int rc = visit(c == 1 ? DotQueriesStep{q, 1, 0, rows, 1, kDotPlainRT} : DotQueriesStep{q, c, 0, rows, tile.QT, tile.RT})) return rc;
  }
  return 0;
}

// The weight table of the weighted sums (Evaluator::multiply_sum with weights; hipbfv_debug_weight_residues prints it): out[t * count + i]
// = {w_t mod primes[i], canonical in [0, q), and its Shoup quotient floor(r * 2^64 / q)}.  Any int32_t is a weight.
inline void weight_residues(const u64* primes, size_t count, const int32_t* weights, size_t terms, MulOp* out) {
  for (size_t t = 0; t < terms; t++)
    for (size_t i = 0; i < count; i++) {
      const u64 q = primes[i];
      const int64_t w = weights[t];
      const u64 m = (u64)(w < 0 ? -w : w) % q;
      const u64 r = w < 0 && m ? q - m : m;
      out[t * count + i] = MulOp{r, (u64)(((unsigned __int128)r << 64) / q)};
    }
}

// Transparent-result watch of the batched path.  While a WatchScope is alive on the calling thread, every Evaluator
// operation that produces ciphertexts records, in the device word it was given, the smallest batch index whose result is
// transparent (all polynomials but the first are zero; 0xFFFFFFFF = none): the reference's SEAL build throws on such a
// result (seal_fhe/build.rs:46-66, sunscreen/tests/features.rs:8-34).  The handle-level C entry points do their own
// per-call check and never open a scope.
struct WatchScope {
  explicit WatchScope(u32* status_dev);
  ~WatchScope();
  u32* prev;
};

class Evaluator {
 public:
  explicit Evaluator(Context* ctx);
  ~Evaluator();
  // the evaluator's own status word for hipbfv_batch_* callers (nullptr if the allocation failed); read-and-reset:
  // *first_bad = smallest transparent item since the last call, 0xFFFFFFFF if none.  Synchronises `s`.
  u32* batch_status() const { return status_dev_; }
  int take_status(u32* status_dev, u32* first_bad, hipStream_t s);
  int note_result(const u64* ct, u32 size, u32 residues, size_t count, hipStream_t s);
  static u32* watch_status();  // the status word of the calling thread's innermost WatchScope (nullptr outside one)
  bool few_for_split_mul(size_t count) const;
  bool few_for_split_ks(size_t count) const;
  bool few_for_fused(size_t count) const;
  Profiler& profiler() { return prof_; }
  ScratchPool& scratch() { return pool_; }
  Context* ctx() const { return ctx_; }

  // ---- SURVEY 8a rows a1-a5, batched ----
  // sh (here, in multiply_relin, multiply_sum and multiply_sum_relin): the second operands are prepared ciphertexts (SharedSel above), b is
  // unused.  The path is the one the call takes without it; where that is the split kernels, the head extends `a` alone and
  // launch_mul_mid_shared reads the prepared rows, elsewhere the chunk's multiplicands are gathered from sh->m->ct.  The same words.
  // pr (the same four): BOTH operands are prepared ciphertexts (PairSel above), a and b are unused.  On the split path there is no head:
  // launch_mul_mid_pair reads both operands' rows and the tail runs unchanged; elsewhere both operands of a chunk are gathered from the
  // objects' canonical copies and the existing launches run.  The same words.  sh and pr exclude each other.
  int multiply(const u64* a, u32 sa, const u64* b, u32 sb, u64* out, size_t count, hipStream_t s, bool watch = true, const SharedSel* sh = nullptr,
               const PairSel* pr = nullptr);
  // addend (optional, the three key-switching operations): ciphertexts u64[count][2][K][N] added to the results inside the last kernel
  // rk / key: one key for the whole batch (a device pointer converts) or a per-item selection (KeySel above)
  int relinearize(const u64* ct3, const KeySel& rk, u64* out2, size_t count, hipStream_t s, const u64* addend = nullptr, bool watch = true);
  // members / per (program executor, merged launches): a DEVICE table of per-member epilogues (kernels.hpp MemberTail) -- item i belongs to
  // member i / per and is written to that member's own buffer as mult * product + sign * extra; out2 and addend are unused then, and
  // the caller notes the results itself.  Only where member_tail_ok(count) says so (the all-FP64 fused path).
  // heads (with members): the members' operands where they are (kernels.hpp MemberHead) -- a and b are unused then, `square` says whether every
  // member multiplies a ciphertext by itself
  int multiply_relin(const u64* a, const u64* b, const KeySel& rk, u64* out2, size_t count, hipStream_t s, const u64* addend = nullptr,
                     const MemberTail* members = nullptr, u32 per = 0, const MemberHead* heads = nullptr, bool heads_square = false,
                     const SharedSel* sh = nullptr, const PairSel* pr = nullptr);
  bool member_tail_ok(size_t count) const;
  // Sums of products with lazy relinearization: a, b = u64[groups][terms][2][K][N] (b == a: sums of squares),
  // out3[g] = sum_t a[g][t] * b[g][t] as size-3 ciphertexts -- word for word the sum of multiply()'s results (the order of a modular
  // sum does not matter), written once per group.  Where multiply() takes the split kernels for groups * terms items, the last of them
  // sums in registers (launch_mul_tail_sum); otherwise multiply() runs into a staging buffer that the element-wise kernel folds.
  // The launch sequences are plan_multiply_sum's over chunk_ops().  A transparent term inside a non-transparent sum is not seen.
  // wt (optional; callers inside the class, which stage it): a DEVICE table MulOp[terms][K] of weights (weight_residues above), shared
  // by every group -- out3[g] = sum_t w_t (.) a[g][t] * b[g][t], the weight applied to the finished canonical residues of a term
  // just before they are added (mul_tail_sum_weighted_kernel; scaled_accumulate_kernel on the folded path).  A slice that starts at
  // term0 reads the table from row term0.
  int multiply_sum(const u64* a, const u64* b, u64* out3, size_t groups, size_t terms, hipStream_t s, bool watch = true, const MulOp* wt = nullptr,
                   const SharedSel* sh = nullptr, const PairSel* pr = nullptr);
  // weights: a HOST array of `terms` entries, read before the call returns and staged once (stage_weights).  All weights 1: the call above.
  int multiply_sum_weighted(const u64* a, const u64* b, const int32_t* weights, u64* out3, size_t groups, size_t terms, hipStream_t s);
  // out2[g] = relinearize(sum_t a[g][t] * b[g][t]): one key switch per GROUP; rk selects per group.  weights (optional): as above,
  // staged once for the whole call, not once per block of groups
  int multiply_sum_relin(const u64* a, const u64* b, const KeySel& rk, u64* out2, size_t groups, size_t terms, hipStream_t s,
                         const int32_t* weights = nullptr, const SharedSel* sh = nullptr, const PairSel* pr = nullptr);
  // Prepared multiplicands: ct2 = u64[count][2][K][N] is copied and, where the parameter set has a split multiply, extended and
  // transformed once (mul_head on two polynomials, mul_prep_mid).  Asynchronous on s; *out is owned by the caller (delete).
  int prepare_multiplicand(const u64* ct2, size_t count, hipStream_t s, Multiplicand** out);
  // kInvalidArg unless sel names an object of this context and every index is below its count (*bad: the first item that is not);
  // nothing is launched
  int check_shared(const SharedSel& sel, size_t items, size_t* bad) const;
  // the four products over prepared multiplicands (include/hipbfv.h, hipbfv_batch_multiply_shared ...): the stream waits for the
  // object's event, then the counterpart's launch sequence runs with sh
  int multiply_shared(const u64* a, const SharedSel& sh, u64* out3, size_t count, hipStream_t s);
  int multiply_relin_shared(const u64* a, const SharedSel& sh, const KeySel& rk, u64* out2, size_t count, hipStream_t s);
  int multiply_sum_shared(const u64* a, const SharedSel& sh, u64* out3, size_t groups, size_t terms, hipStream_t s);
  int multiply_sum_relin_shared(const u64* a, const SharedSel& sh, const KeySel& rk, u64* out2, size_t groups, size_t terms, hipStream_t s);
  // kInvalidArg unless both objects belong to this context and every index is below its object's count (*bad: the first item that is
  // not, *bad_b: whether it is the second operand's index); nothing is launched
  int check_pair(const PairSel& sel, size_t items, size_t* bad, bool* bad_b) const;
  // the four products of two prepared operands (include/hipbfv.h, hipbfv_batch_multiply_prepared ...): the stream waits for both
  // objects' events, then the counterpart's launch sequence runs with pr
  int multiply_prepared(const PairSel& pr, u64* out3, size_t count, hipStream_t s);
  int multiply_relin_prepared(const PairSel& pr, const KeySel& rk, u64* out2, size_t count, hipStream_t s);
  int multiply_sum_prepared(const PairSel& pr, u64* out3, size_t groups, size_t terms, hipStream_t s);
  int multiply_sum_relin_prepared(const PairSel& pr, const KeySel& rk, u64* out2, size_t groups, size_t terms, hipStream_t s);
  // out2 = (sigma_g(c0), 0) + switch_key(sigma_g(c1), key)
  int apply_galois(const u64* ct2, u32 galois_elt, const KeySel& key, u64* out2, size_t count, hipStream_t s, const u64* addend = nullptr);
  // every item by its OWN Galois element in one key-switch pass (mixed-step rotation batches): elts / keys are HOST arrays of `count`
  // entries, keys[i] the device key of elts[i] (not read for the elements 0 and 1).  Element 1: the item is copied.  Element 0
  // (callers inside the library only: items another pass produces): the item is left out, out2[i] is not written.  Everything
  // is validated before the first launch.  watch = false: the caller notes the results itself (it fills the left-out items first).
  int apply_galois_items(const u64* ct2, const u32* elts, const u64* const* keys, u64* out2, size_t count, hipStream_t s, bool watch = true);
  // ... with one key set per client (evaluator_client.cpp): keys[i] may differ between items of one element, the key table has one entry
  // per (key, element) pair and the walk is ordered by (element, key).  apply_galois_items above keys its table by element alone -- its
  // callers hand it ONE key set.  key_ids (optional, host, `count` entries): the number of item i's key set, equal for equal keys --
  // it orders the keys of one element (without it: the order in which the key pointers first appear).
  int apply_galois_items_keyed(const u64* ct2, const u32* elts, const u64* const* keys, const u32* key_ids, u64* out2, size_t count, hipStream_t s,
                               bool watch = true);
  // NAF chains in shared rounds: batch item items[j] (j < nitems) through the elements elts[r * nitems + j], r < rounds (0: the item has
  // finished), each through keys[r * nitems + j]; one gather, one apply_galois_items_keyed call per round between two stages, the items
  // scattered to out2 from the stage they finished in.  Host arrays; the results are not noted (the caller does).
  int apply_galois_rounds(const u64* ct2, u64* out2, const u64* items, size_t nitems, u32 rounds, const u32* elts, const u64* const* keys,
                          const u32* key_ids, hipStream_t s);
  // Sums of rotations: out2[g] (u64[groups][2][K][N]) = the sum over t < terms of apply_galois(items[g * terms + t].src, .elt), word for
  // word what apply_galois + add give in any order.  items: a HOST array of groups * terms entries -- src: the term's source ciphertext
  // (device, u64[2][K][N]; many items may name one), elt: its Galois element (1: the source itself enters the sum), key: the device key
  // of elt (not read for element 1).  No source may overlap out2.  Everything is validated before the first launch.
  // Where the split kernels run (ks_split_for(groups * terms), fused automorphisms, N = 4096 ... 16384) every launch sequence of
  // plan_multiply_sum over chunk_ops() is ONE ks_head_src -> ks_mid -> ks_tail_sum: a term is finished and added inside the last kernel
  // and never written.  Elsewhere a sequence's terms are gathered, rotated by apply_galois_items into a stage and folded by the
  // element-wise add.  The sums are noted under GROUP numbers; a transparent term inside a sum that is not transparent is not seen.
  struct RotSumItem {
    const u64* src;
    u32 elt;
    const u64* key;
  };
  // weights (optional): a HOST array of `terms` int32_t shared by every group, read before the call returns and staged once on s
  // (stage_weights, as multiply_sum_weighted's) -- out2[g] = sum_t w_t (.) apply_galois(...), every finished canonical residue of term t,
  // row i multiplied by (w_t mod q_i) just before it is added: in ks_tail_sum_weighted_kernel on the split path (a slice that starts at
  // term0 reads the table from row term0), by one scaled_accumulate per term and group elsewhere.  Identity terms are weighted as any
  // other; a zero weight is a weight like any other.  All weights 1: the unweighted launches.
  int rotate_sum(const RotSumItem* items, u64* out2, size_t groups, size_t terms, hipStream_t s, const int32_t* weights = nullptr);
  int mod_switch_next(const u64* ct, u32 size, u64* out, size_t count, hipStream_t s);  // out has K-1 residues per polynomial
  int add(const u64* a, const u64* b, u64* out, u32 size, size_t count, hipStream_t s);
  int sub(const u64* a, const u64* b, u64* out, u32 size, size_t count, hipStream_t s);
  int negate(const u64* a, u64* out, u32 size, size_t count, hipStream_t s);
  // plain: u64[count][N] (pstride = N) or one shared plaintext (pstride = 0), coefficients < t, zero padded
  int add_plain(const u64* ct, u32 size, const u64* plain, size_t pstride, u64* out, size_t count, hipStream_t s);
  int sub_plain(const u64* ct, u32 size, const u64* plain, size_t pstride, u64* out, size_t count, hipStream_t s);
  int multiply_plain(const u64* ct, u32 size, const u64* plain, size_t pstride, u64* out, size_t count, hipStream_t s);
  // monomial fast path of SEAL multiply_plain_normal: plaintext = coeff * x^exponent
  int multiply_plain_mono(const u64* ct, u32 size, u64 coeff, u32 exponent, u64* out, size_t count, hipStream_t s);
  // flags[i] = 1 if ciphertext i is NOT transparent (some word of polys 1.. is non-zero); flags must be zeroed
  int nonzero_tail(const u64* ct, u32 size, u32* flags, size_t count, hipStream_t s);

  // ---- the steps either side of the path (evaluator_client.cpp) ----
  int batch_encode(const u64* values, u64* plain, size_t count, bool is_signed, u32* bad_host, hipStream_t s);
  int batch_decode(const u64* plain, u64* values, size_t count, bool is_signed, hipStream_t s);
  // plain (u64[count][N]) and / or noise: the plaintexts, the invariant-noise measure, or both from one phase computation
  int decrypt(const u64* ct, u32 size, const u64* sk_ntt, u64* plain, size_t count, hipStream_t s, const NoiseOut* noise = nullptr);
  int keygen_secret(const RngSeed& seed, u64* sk_coeff, u64* sk_ntt, hipStream_t s);
  int keygen_zero_encryptions(const RngSeed& seed, u64 stream, const u64* sk_ntt, const u64* w, u64* key, u32 count, hipStream_t s);
  // single encryptions that also return the sampled polynomials (fork-only API used by logproof), and secret-key encryption
  int encrypt_components(const u64* plain, const u64* pk, const RngSeed& seed, u64 op, bool no_special, u64* ct2, u64* u_out, u64* e_out, hipStream_t s);
  int encrypt_symmetric(const u64* plain, const u64* sk_ntt, const RngSeed& seed, u64 stream, u64* ct2, u64* e_out, hipStream_t s);
  int key_to_coeff(const u64* key, u32 polys, u64* out, hipStream_t s);
  int crt_compose(const u64* consts, u32 kc, const u64* in, u64* out, u32 polys, hipStream_t s);
  int crt_decompose(u32 kc, const u64* in, u64* out, u32 polys, hipStream_t s);
  int keygen_kswitch(const RngSeed& seed, u64 stream, const u64* sk_coeff, const u64* sk_ntt, u32 galois_elt, u64* key, hipStream_t s);
  int keygen_galois_poly(const u64* sk_coeff, u32 galois_elt, u64* out, hipStream_t s);
  // watch_zero: an all-zero plaintext raises the transparent-result status of the enclosing WatchScope -- 1: the plaintexts are
  // the items of a batch (item = index), 2: they are shared by the whole batch (item 0): the graph executor's transform-domain
  // sums never form the single product SEAL's multiply_plain would have refused
  int plain_to_ntt(const u64* plain, size_t pstride, u64* pntt, size_t count, hipStream_t s, int watch_zero = 0);
  int ct_to_ntt(const u64* ct, u32 size, u64* ctn, size_t count, hipStream_t s);
  int dot_plain_ntt(const u64* ctn, u32 cols, const u64* pntt, u32 rows, u64* out, hipStream_t s);
  // `queries` queries against ONE database pass: ctn u64[queries][cols][2][K][N], out u64[queries][rows][2][K][N], out[q] word for
  // word dot_plain_ntt(ctn + q * cols * 2 * K * N).  The product launches are plan_dot_queries' (one, in practice).
  int dot_plain_ntt_queries(const u64* ctn, u32 queries, u32 cols, const u64* pntt, u32 rows, u64* out, hipStream_t s);
  // the graph executor's form: ctn u64[cols][batch][2][K][N] (transform domain), tab [rows][cols] device descriptors of
  // transform-domain plaintexts, out u64[rows][batch][2][K][N] in coefficient form
  int dot_plain_tab(const u64* ctn, u32 cols, const PlainNttRef* tab, u32 rows, u32 batch, u64* out, hipStream_t s);
  // ct (.) plaintext given in transform form (u64[K][N] at pntt + item * pnstride): transform, product, inverse transform
  int multiply_plain_ntt(const u64* ct, u32 size, const u64* pntt, size_t pnstride, u64* out, size_t count, hipStream_t s);
  // the transparent-result watch of one n-ary sum launch (device descriptor table)
  int note_nary(const NaryOut* douts, u32 nouts, u32 batch, hipStream_t s);
  int encrypt(const u64* plain, size_t pstride, const u64* pk, const RngSeed& seed, u64 first_op, u64* ct2, size_t count, hipStream_t s);

  // ---- NTT entry points (BASELINE config 2) ----
  // data: u64[polys][N]; polynomial p uses key-level prime (p % nprimes)
  int ntt(u64* data, size_t polys, u32 nprimes, bool inverse, hipStream_t s);

  u32 galois_elt_from_step(int step) const;  // 0 if |step| >= n/2
  static u32 galois_elt_from_step(u32 n, int step);
  size_t chunk_ops() const { return chunk_ops_; }
  void set_chunk_ops(size_t c) { chunk_ops_ = c ? c : 1; }

 private:
  int key_switch(const u64* target, size_t tstride, const u64* key, const u64* base, size_t bstride, u32 base_mask, u64* out2,
                 size_t count, u64* scratch, hipStream_t s, const u64* extra = nullptr, KeyMap km = KeyMap{}, u32 ginv = 0,
                 const u32* ginv_tab = nullptr);
  bool ks_split_for(size_t count) const;  // key_switch takes the head / middle / tail kernels for a batch of this size
  size_t ks_scratch_words() const;
  // the device tables of a per-item key selection for one call: `order` holds, for every chunk of `chunk` items, the chunk's items
  // (numbered from 0 within the chunk) sorted by key -- the launch over chunk c reads order + c * chunk
  struct KeyMapLease {
    Evaluator* ev = nullptr;
    hipStream_t s = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    KeyMap km;
    const u32* words = nullptr;  // device copy of stage_keymap's item_words
    KeyMap at(size_t off) const { return km.keys ? KeyMap{km.keys, km.order + off} : KeyMap{}; }
    ~KeyMapLease();
  };
  // item_words (optional): one u32 per item of the call, staged behind the tables with the same copy (the per-item g^-1 of
  // apply_galois_items).  With it an index of kKeyNone is allowed: the item takes no key -- it is listed last in its chunk's order, as
  // item 0xFFFFFFFF, which the middle kernels drop.
  static constexpr u32 kKeyNone = 0xFFFFFFFFu;
  int stage_keymap(const KeySel& sel, size_t count, size_t chunk, hipStream_t s, KeyMapLease& lease, const u32* item_words = nullptr);
  // the device weight table of one weighted call: a pinned block and one H2D copy on the call's stream, as stage_keymap's; both
  // buffers go back to their pools behind the call's last launch.  wt stays nullptr when every weight is 1 (the unweighted launches).
  struct WeightLease {
    Evaluator* ev = nullptr;
    hipStream_t s = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    const MulOp* wt = nullptr;
    ~WeightLease();
  };
  int stage_weights(const int32_t* weights, size_t terms, hipStream_t s, WeightLease& lease);
  // the device tables of one rotate_sum call on the split path, staged as stage_keymap's: the key table, every launch sequence's items
  // sorted by key (numbered from 0 within the sequence, at order + the sequence's first item) and the RotTerm entry of every item
  struct RotSumLease {
    Evaluator* ev = nullptr;
    hipStream_t s = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    KeyMap km;
    const RotTerm* terms = nullptr;
    ~RotSumLease();
  };
  // the device table of one call over prepared multiplicands, staged as stage_keymap's: rows -- u32[items], item i's index (the split
  // path: launch_mul_mid_shared reads idx + first item of the launch); otherwise a pointer table, item i's canonical ciphertext
  // (launch_gather_items)
  struct SharedLease {
    Evaluator* ev = nullptr;
    hipStream_t s = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    const u32* idx = nullptr;
    const u64* const* ptrs = nullptr;
    ~SharedLease();
  };
  int stage_shared(const SharedSel& sel, size_t items, bool rows, hipStream_t s, SharedLease& lease);
  // ... of one call over two prepared operands: rows -- uint2[items], item i's {a, b} indices (launch_mul_mid_pair reads idx + first item
  // of the launch); otherwise two pointer tables of `items` entries each, item i's canonical ciphertexts (launch_gather_items)
  struct PairLease {
    Evaluator* ev = nullptr;
    hipStream_t s = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    const uint2* idx = nullptr;
    const u64* const* ptrs_a = nullptr;
    const u64* const* ptrs_b = nullptr;
    ~PairLease();
  };
  int stage_pair(const PairSel& sel, size_t items, bool rows, hipStream_t s, PairLease& lease);
  bool split_mul_params() const;  // the parameter set has a split multiply at all (multiply()'s conditions but the item count)
  PinnedPool pinned_;
  Context* ctx_;
  u32* status_dev_ = nullptr;
  ScratchPool pool_;
  Profiler prof_;
  size_t chunk_ops_;
  bool split_ks_ = true;   // head / middle / tail split transforms for key switching (kernels_split.hip)
  bool split_mul_ = true;  // ... and for the BEHZ multiply
  bool fuse_head_ = true;      // ... and c2 formed inside the key switch's first kernel
  bool small_batch_ = true;    // a few ciphertexts take the whole-polynomial pipelines (HIPBFV_NO_SMALL_BATCH=1: pipelines chosen by parameters only)
  bool fuse_galois_ = true;    // rotations: the automorphism read through the key switch's head / tail loads (no rotated copy)
  bool fuse_mulrelin_ = true;  // multiply_relin: c0, c1 of the product formed inside the key switch's last kernel
};

// How a row rotation by `step` runs over one holding of Galois keys (SEAL's Evaluator::rotate_internal), decided on the host before
// anything is launched: through the step's own key when it is held, otherwise through the chain of power-of-two rotations of the
// step's non-adjacent form (NAF), least significant digit first, the sign carried by every part.  A part of n/2 rows is the identity
// on the rows and is no hop.  hop[0, hops) are the Galois elements to apply in order: the step's own for kDirect, none for kCopy.
struct RowRotation {
  enum Kind : int32_t { kCopy = 0, kDirect = 1, kChain = 2, kTooLarge = 3, kNoKey = 4 };  // kTooLarge, kNoKey: refused
  Kind kind = kCopy;
  u32 elt = 1;      // the step's own Galois element (0: kTooLarge)
  u32 missing = 0;  // kNoKey: the element whose key was looked for and not found
  u32 hops = 0;
  u32 hop[32];
};

// has(element): the holding has that element's key.  A chain needs two NAF parts or more: a power of two without its key is kNoKey.
template <class Has>
RowRotation plan_row_rotation(u32 n, int step, Has&& has) {
  RowRotation r;
  if (step == 0) return r;
  r.elt = Evaluator::galois_elt_from_step(n, step);  // refuses |step| >= n/2 (INT_MIN too) before the step is negated below
  const auto refused = [&](RowRotation::Kind why, u32 missing) {
    r.kind = why, r.missing = missing, r.hops = 0;
    return r;
  };
  if (!r.elt) return refused(RowRotation::kTooLarge, 0);
  if (has(r.elt)) {
    r.kind = RowRotation::kDirect, r.hop[r.hops++] = r.elt;
    return r;
  }
  u32 parts = 0;
  int v = step < 0 ? -step : step;
  for (int i = 0; v; i++) {
    const int zi = (v & 1) ? 2 - (v & 3) : 0;
    v = (v - zi) >> 1;
    if (!zi) continue;
    parts++;
    if ((1u << i) == (n >> 1)) continue;
    r.hop[r.hops++] = Evaluator::galois_elt_from_step(n, (step < 0 ? -zi : zi) * (1 << i));
  }
  if (parts < 2) return refused(RowRotation::kNoKey, r.elt);
  for (u32 h = 0; h < r.hops; h++)
    if (!has(r.hop[h])) return refused(RowRotation::kNoKey, r.hop[h]);
  r.kind = RowRotation::kChain;
  return r;
}

// The launches of an accepted plan: hop(element, cur, out) per hop, cur = in first and out afterwards; the first non-zero status ends it.
template <class In, class Out, class Hop>
auto run_row_rotation(const RowRotation& r, In in, Out out, Hop&& hop) -> decltype(hop(0u, in, out)) {
  In cur = in;
  for (u32 h = 0; h < r.hops; h++) {
    if (auto st = hop(r.hop[h], cur, out)) return st;
    cur = out;
  }
  return 0;
}

}  // namespace hipbfv
