// sunscreen_amd/csrc/capi_shared.hpp -- the C entry points of the prepared multiplicands (include/hipbfv.h: hipbfv_Multiplicand_*,
// hipbfv_batch_multiply*_shared, hipbfv_batch_multiply*_prepared).  Part of capi.cpp's translation unit (included at its end, as pool.hpp is): it uses that file's handle
// objects, its exception barrier and its aliasing check.
#pragma once

namespace {

constexpr uint32_t kMagicMultiplicand = 0x4D504C31;

struct MultiplicandObj : Obj {
  std::shared_ptr<Context> ctx;  // keeps the tables the object was made with alive
  std::unique_ptr<Multiplicand> m;
  MultiplicandObj() : Obj(kMagicMultiplicand) {}
};

// the checks the four products share, in the header's order; everything is decided before anything is launched or written
// (terms: 1 for the item-wise calls; exact_ok: the output may be exactly a)
long shared_args(EvalObj* e, const void* a, void* multiplicand, const uint32_t* b_index, uint64_t index_len, const void* out, u32 out_size, uint64_t groups,
                 uint64_t terms, bool exact_ok, SharedSel* sel) {
  MultiplicandObj* mo = as<MultiplicandObj>(multiplicand, kMagicMultiplicand);
  if (!a || !out || !mo || !b_index) return HIPBFV_E_POINTER;
  if (!terms) return fail(HIPBFV_E_INVALIDARG, "a sum of products needs at least one term per group");
  if (groups > 0xFFFFFFFFull || terms > 0xFFFFFFFFull) return fail(HIPBFV_E_INVALIDARG, "too many items, groups or terms");
  if (!index_len) return fail(HIPBFV_E_INVALIDARG, "b_index needs at least one entry");
  if (mo->ctx.get() != e->ctx.get()) return fail(HIPBFV_E_INVALIDARG, "the multiplicand was prepared for another context");
  *sel = SharedSel{mo->m.get(), b_index, (size_t)index_len, 0};
  size_t bad = 0;
  if (e->ev->check_shared(*sel, (size_t)(groups * terms), &bad) != kOk) {
    char msg[160];
    snprintf(msg, sizeof(msg), "item %llu names prepared ciphertext %u of %llu", (unsigned long long)bad, b_index[bad % index_len],
             (unsigned long long)mo->m->count);
    return fail(HIPBFV_E_INVALIDARG, msg);
  }
  return check_alias(cts(out, e->ctx->ct_words(out_size), groups), {cts(a, e->ctx->ct_words(2), groups * terms)}, exact_ok);
}

// ... of the four products of two prepared operands (the objects own the operands: no aliasing rule)
long prepared_args(EvalObj* e, void* ma, const uint32_t* a_index, void* mb, const uint32_t* b_index, uint64_t index_len, const void* out, uint64_t groups,
                   uint64_t terms, PairSel* sel) {
  MultiplicandObj* oa = as<MultiplicandObj>(ma, kMagicMultiplicand);
  MultiplicandObj* ob = as<MultiplicandObj>(mb, kMagicMultiplicand);
  if (!out || !oa || !ob || !a_index || !b_index) return HIPBFV_E_POINTER;
  if (!terms) return fail(HIPBFV_E_INVALIDARG, "a sum of products needs at least one term per group");
  if (groups > 0xFFFFFFFFull || terms > 0xFFFFFFFFull) return fail(HIPBFV_E_INVALIDARG, "too many items, groups or terms");
  if (!index_len) return fail(HIPBFV_E_INVALIDARG, "a_index and b_index need at least one entry");
  if (oa->ctx.get() != e->ctx.get() || ob->ctx.get() != e->ctx.get())
    return fail(HIPBFV_E_INVALIDARG, "a multiplicand was prepared for another context");
  *sel = PairSel{oa->m.get(), ob->m.get(), a_index, b_index, (size_t)index_len, 0};
  size_t bad = 0;
  bool bad_b = false;
  if (e->ev->check_pair(*sel, (size_t)(groups * terms), &bad, &bad_b) != kOk) {
    char msg[160];
    snprintf(msg, sizeof(msg), "item %llu: %s names prepared ciphertext %u of %llu", (unsigned long long)bad, bad_b ? "b_index" : "a_index",
             (bad_b ? b_index : a_index)[bad % index_len], (unsigned long long)(bad_b ? ob : oa)->m->count);
    return fail(HIPBFV_E_INVALIDARG, msg);
  }
  return HIPBFV_S_OK;
}

MultiplicandObj* multiplicand_of(void* h) { return as<MultiplicandObj>(h, kMagicMultiplicand); }

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

long hipbfv_Multiplicand_Create(void* h, const uint64_t* ct2, uint64_t count, void* stream, void** multiplicand) HIPBFV_BEGIN
  EvalObj* e = as<EvalObj>(h, kMagicEval);
  if (!e || !ct2 || !multiplicand) return HIPBFV_E_POINTER;
  if (!count || count > 0xFFFFFFFFull) return fail(HIPBFV_E_INVALIDARG, "a multiplicand holds 1 to 2^32 - 1 ciphertexts");
  std::unique_ptr<MultiplicandObj> mo(new MultiplicandObj());
  mo->ctx = e->ctx;
  Multiplicand* m = nullptr;
  if (int rc = e->ev->prepare_multiplicand((const u64*)ct2, (size_t)count, (hipStream_t)stream, &m)) return from_status(rc);
  mo->m.reset(m);
  *multiplicand = mo.release();
  return HIPBFV_S_OK;
HIPBFV_END

long hipbfv_Multiplicand_Destroy(void* multiplicand) HIPBFV_BEGIN
  MultiplicandObj* mo = multiplicand_of(multiplicand);
  if (!mo) return HIPBFV_E_POINTER;
  delete mo;
  return HIPBFV_S_OK;
HIPBFV_END

long hipbfv_Multiplicand_Count(void* multiplicand, uint64_t* count) HIPBFV_BEGIN
  MultiplicandObj* mo = multiplicand_of(multiplicand);
  if (!mo || !count) return HIPBFV_E_POINTER;
  *count = mo->m->count;
  return HIPBFV_S_OK;
HIPBFV_END

long hipbfv_Multiplicand_Bytes(void* multiplicand, uint64_t* bytes) HIPBFV_BEGIN
  MultiplicandObj* mo = multiplicand_of(multiplicand);
  if (!mo || !bytes) return HIPBFV_E_POINTER;
  *bytes = mo->m->bytes;
  return HIPBFV_S_OK;
HIPBFV_END

long hipbfv_batch_multiply_shared(void* h, const uint64_t* a, void* multiplicand, const uint32_t* b_index, uint64_t index_len, uint64_t* out3,
                                  uint64_t count, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  SharedSel sel;
  if (long hr = shared_args(e, a, multiplicand, b_index, index_len, out3, 3, count, 1, false, &sel)) return hr;
  if (!count) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_shared((const u64*)a, sel, (u64*)out3, count, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_relin_shared(void* h, const uint64_t* a, void* multiplicand, const uint32_t* b_index, uint64_t index_len, void* relin_keys,
                                        uint64_t* out2, uint64_t count, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  SharedSel sel;
  if (long hr = shared_args(e, a, multiplicand, b_index, index_len, out2, 2, count, 1, true, &sel)) return hr;
  const u64* rk = key_or_null(relin_keys, e, 0);
  if (!rk) return from_status(kNoKey);
  if (!count) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_relin_shared((const u64*)a, sel, rk, (u64*)out2, count, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_sum_shared(void* h, const uint64_t* a, void* multiplicand, const uint32_t* b_index, uint64_t index_len, uint64_t* out3,
                                      uint64_t groups, uint64_t terms, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  SharedSel sel;
  if (long hr = shared_args(e, a, multiplicand, b_index, index_len, out3, 3, groups, terms, false, &sel)) return hr;
  if (!groups) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_sum_shared((const u64*)a, sel, (u64*)out3, groups, terms, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_sum_relin_shared(void* h, const uint64_t* a, void* multiplicand, const uint32_t* b_index, uint64_t index_len, void* relin_keys,
                                            uint64_t* out2, uint64_t groups, uint64_t terms, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  SharedSel sel;
  if (long hr = shared_args(e, a, multiplicand, b_index, index_len, out2, 2, groups, terms, false, &sel)) return hr;
  const u64* rk = key_or_null(relin_keys, e, 0);
  if (!rk) return from_status(kNoKey);
  if (!groups) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_sum_relin_shared((const u64*)a, sel, rk, (u64*)out2, groups, terms, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_prepared(void* h, void* ma, const uint32_t* a_index, void* mb, const uint32_t* b_index, uint64_t index_len, uint64_t* out3,
                                    uint64_t count, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  PairSel sel;
  if (long hr = prepared_args(e, ma, a_index, mb, b_index, index_len, out3, count, 1, &sel)) return hr;
  if (!count) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_prepared(sel, (u64*)out3, count, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_relin_prepared(void* h, void* ma, const uint32_t* a_index, void* mb, const uint32_t* b_index, uint64_t index_len,
                                          void* relin_keys, uint64_t* out2, uint64_t count, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  PairSel sel;
  if (long hr = prepared_args(e, ma, a_index, mb, b_index, index_len, out2, count, 1, &sel)) return hr;
  const u64* rk = key_or_null(relin_keys, e, 0);
  if (!rk) return from_status(kNoKey);
  if (!count) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_relin_prepared(sel, rk, (u64*)out2, count, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_sum_prepared(void* h, void* ma, const uint32_t* a_index, void* mb, const uint32_t* b_index, uint64_t index_len, uint64_t* out3,
                                        uint64_t groups, uint64_t terms, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  PairSel sel;
  if (long hr = prepared_args(e, ma, a_index, mb, b_index, index_len, out3, groups, terms, &sel)) return hr;
  if (!groups) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_sum_prepared(sel, (u64*)out3, groups, terms, (hipStream_t)stream));
HIPBFV_END

long hipbfv_batch_multiply_sum_relin_prepared(void* h, void* ma, const uint32_t* a_index, void* mb, const uint32_t* b_index, uint64_t index_len,
                                              void* relin_keys, uint64_t* out2, uint64_t groups, uint64_t terms, void* stream) HIPBFV_BEGIN
  EVAL_OR_RETURN(h);
  PairSel sel;
  if (long hr = prepared_args(e, ma, a_index, mb, b_index, index_len, out2, groups, terms, &sel)) return hr;
  const u64* rk = key_or_null(relin_keys, e, 0);
  if (!rk) return from_status(kNoKey);
  if (!groups) return HIPBFV_S_OK;
  return from_status(e->ev->multiply_sum_relin_prepared(sel, rk, (u64*)out2, groups, terms, (hipStream_t)stream));
HIPBFV_END

}  // extern "C"
#pragma GCC visibility pop
