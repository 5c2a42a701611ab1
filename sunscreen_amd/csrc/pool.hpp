// sunscreen_amd/csrc/pool.hpp -- the device pool behind hipbfv_Pool_* (include/hipbfv.h, "Device pool").
//
// Included by capi.cpp only, after the handle objects (KeysObj, EvalObj, ProgramObj) and program_run_impl that it drives.
//
// A pool is a list of members.  A member is one device with its own Context (built from the pool's parameters), Evaluator,
// three streams (in / compute / out), three pipeline slots of device memory, pinned bounce buffers for pageable host memory,
// a cache of key copies (optionally bounded: hipbfv_Pool_SetKeyCacheBytes) and ONE worker thread that sets its device once and does all of the member's HIP work: every
// thread-local cache it touches (program_plan.cpp's stream tables and TableArenas, the evaluator's watch scope) stays on
// that device.  A call shards the batch as sunscreen_amd/dist.py:shard_range does, hands every non-empty shard to its
// member's worker and waits for all of them.  No new kernel: each member runs the library's own launch sequences.
//
// Per-client key sets (hipbfv_Pool_*Keys): the calling thread validates every referenced set over the whole batch and lists,
// per set, the key buffers the call needs (PoolSetKeys).  On the member, every chunk gets its own key table (pool_keyplan: the
// distinct sets of the chunk, key_index remapped onto them), the member copies just those sets' needed buffers
// (member_stage_keys) and hands the library's per-key entry points views of its own context (member_chunk_keys).
#pragma once

namespace {

constexpr uint32_t kMagicPool = 0x504F4F31;
constexpr int kPoolSlots = 3;  // chunks in flight per member: one copying in, one computing, one copying out

// dist.py:shard_range: contiguous blocks whose sizes differ by at most one
void pool_shard(u64 total, u64 members, u64 r, u64* lo, u64* hi) {
  const u64 base = total / members, extra = total % members;
  *lo = r * base + std::min<u64>(r, extra);
  *hi = *lo + base + (r < extra ? 1 : 0);
}

// 0 = the library's choice: 2^21 / N input sets (256 at N = 8192, 128 at N = 16384: the sizes the PCIe note measured)
u64 pool_default_chunk(u32 n) { return std::max<u64>(16, std::min<u64>(1024, ((u64)1 << 21) / n)); }

enum class HostMem { kPageable, kPinned, kDevice };
// What hipPointerGetAttributes says about the first and the last byte of a host operand
HostMem host_kind(const void* p, size_t bytes) {
  if (!p || !bytes) return HostMem::kPageable;
  bool pinned = true;
  for (const char* q : {(const char*)p, (const char*)p + bytes - 1}) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // ordinary pageable memory is an error on some runtimes, "unregistered" on others
      pinned = false;
      continue;
    }
    if (a.type == hipMemoryTypeHost) continue;
    if (a.type != hipMemoryTypeUnregistered || a.isManaged) return HostMem::kDevice;
    pinned = false;
  }
  return pinned ? HostMem::kPinned : HostMem::kPageable;
}

// One operand of a call in host memory: `width` words per input set, `stride` words apart (stride 0: one item shared by every set)
struct PoolIn {
  const u64* host;
  size_t width, stride;
  bool pinned;
};
struct PoolOut {
  u64* host;
  size_t width;
  bool pinned;
};

// A key buffer of a handle as the call found it (read on the calling thread)
struct PoolKey {
  u32 index;
  u64 stamp;
  const u64* src;
  int src_device;
  size_t words;
};

// What a call needs of every key set of the caller's array (empty for a set no input set names), read on the calling thread
struct PoolSetKeys {
  std::vector<std::vector<PoolKey>> relin, galois;  // [caller's set]
};

// A member's copy of one key buffer
struct PoolKeyCopy {
  u64* dev;
  size_t bytes;
  u64 tick;  // member's key_tick when a chunk last referenced it (least recently used goes first)
};

// A key handle of the member's context whose buffers the key cache owns: nothing goes to g_buffers when it dies
struct PoolKeyView : KeysObj {
  ~PoolKeyView() override {
    keys.clear();
    stamps.clear();
  }
};

// The key table of one chunk: the distinct sets key_index[0, count) names, ascending in the caller's numbering, and the
// chunk's key_index remapped onto them (hipbfv_debug_pool_keyplan shows exactly this)
void pool_keyplan(const uint32_t* key_index, u64 count, std::vector<uint32_t>* sets, std::vector<uint32_t>* remapped) {
  sets->assign(key_index, key_index + count);
  std::sort(sets->begin(), sets->end());
  sets->erase(std::unique(sets->begin(), sets->end()), sets->end());
  remapped->resize(count);
  for (u64 i = 0; i < count; i++)
    (*remapped)[i] = (uint32_t)(std::lower_bound(sets->begin(), sets->end(), key_index[i]) - sets->begin());
}

// A chunk's keys as the per-key entry points take them: handles of the member's context and the remapped key_index
struct PoolChunkKeys {
  std::vector<uint32_t> sets, index;
  std::vector<void*> relin, galois;  // [local set]; NULL where the call needs no such key of the set
};

struct PoolMember {
  int device = 0;
  std::shared_ptr<Context> ctx;  // not counted in g_live_contexts: hipbfv_set_device does not see pool members
  EvalObj eval;                  // the member's evaluator, as the handle object program_run_impl takes
  hipStream_t in = nullptr, comp = nullptr, out = nullptr;
  hipEvent_t in_done[kPoolSlots] = {}, comp_done[kPoolSlots] = {}, out_done[kPoolSlots] = {};
  u64* dev[kPoolSlots] = {};     // per slot: the chunk's inputs, then its outputs
  size_t dev_words = 0;
  u64* bounce[kPoolSlots] = {};  // pinned, the same layout as dev[]: pageable operands pass through it
  size_t bounce_words = 0;
  u64* shared = nullptr;         // the call's shared plaintexts
  size_t shared_words = 0;
  u32* status = nullptr;         // device: the transparent-result word of every chunk (multiply_relin), read once per call
  size_t status_cap = 0;         // words
  u32* flags = nullptr;          // pinned: their host copy
  size_t flag_cap = 0;
  std::map<u64, PoolKeyCopy> key_copy;  // key stamp -> this member's copy (hipMalloc'd here, never from g_buffers)
  u64 key_copies = 0, key_bytes = 0, key_evictions = 0, key_tick = 0;
  KeysObj relin_view, galois_view;  // the call's keys as handles of this member's context (buffers owned by key_copy)
  std::vector<std::unique_ptr<PoolKeyView>> set_relin, set_galois;  // the current chunk's key table ([local set], reused)
  // the worker thread and its one-job mailbox
  std::thread thread;
  std::mutex mu;
  std::condition_variable cv;
  std::function<long()> job;
  bool has_job = false, done = false, quit = false;
  long result = HIPBFV_S_OK;
  std::string message;
};

void pool_worker(PoolMember* m) {
  if (hipSetDevice(m->device) != hipSuccess) (void)hipGetLastError();  // once: everything this thread does stays on the device
  for (;;) {
    std::function<long()> job;
    {
      std::unique_lock<std::mutex> g(m->mu);
      m->cv.wait(g, [&] { return m->has_job || m->quit; });
      if (!m->has_job) return;
      job = std::move(m->job);
      m->has_job = false;
    }
    tls_error.clear();
    long hr;
    try {
      hr = job();
    } catch (const std::bad_alloc&) {
      hr = fail(HIPBFV_E_OUTOFMEMORY, "out of host memory");
    } catch (const std::exception& x) {
      hr = fail(HIPBFV_E_UNEXPECTED, x.what());
    }
    {
      std::lock_guard<std::mutex> g(m->mu);
      m->result = hr;
      m->message = hr != HIPBFV_S_OK ? tls_error : std::string();  // the worker's tls_error, carried back to the caller
      m->done = true;
    }
    m->cv.notify_all();
  }
}

void pool_submit(PoolMember& m, std::function<long()> job) {
  {
    std::lock_guard<std::mutex> g(m.mu);
    m.job = std::move(job);
    m.has_job = true;
    m.done = false;
  }
  m.cv.notify_all();
}

long pool_wait(PoolMember& m, std::string* message) {
  std::unique_lock<std::mutex> g(m.mu);
  m.cv.wait(g, [&] { return m.done; });
  *message = m.message;
  return m.result;
}

struct PoolObj : Obj {
  u32 n = 0, K = 0;  // the parameters every member was built from (the context handle itself is not kept)
  u64 t = 0;
  std::vector<u64> primes;
  std::vector<std::unique_ptr<PoolMember>> members;
  u64 chunk = 0;  // 0 = pool_default_chunk
  u64 key_cache_bytes = 0;  // per member; 0 = no bound
  std::mutex mu;  // one call at a time
  PoolObj() : Obj(kMagicPool) {}
  u64 chunk_sets() const { return chunk ? chunk : pool_default_chunk(n); }
  size_t ct_words() const { return 2 * (size_t)K * n; }  // one size-2 ciphertext
  bool same_params(const Context& c) const { return c.n() == n && c.t() == t && c.key_primes() == primes; }
};

// ---- on the member's worker thread ----
long member_init(PoolMember& m, const PoolObj& p) {
  std::string err;
  Context* c = Context::create(p.n, p.primes, p.t, m.device, &err);
  if (!c) return fail(HIPBFV_E_INVALIDARG, err.c_str());
  m.ctx.reset(c);
  m.eval.ctx = m.ctx;
  m.eval.ev.reset(new Evaluator(c));
  m.relin_view.ctx = m.galois_view.ctx = m.ctx;
  for (hipStream_t* s : {&m.in, &m.comp, &m.out})
    if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) return from_status(kHipError);
  for (int i = 0; i < kPoolSlots; i++)
    for (hipEvent_t* e : {&m.in_done[i], &m.comp_done[i], &m.out_done[i]})
      if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return from_status(kHipError);
  return HIPBFV_S_OK;
}

void member_release(PoolMember& m) {
  for (hipStream_t s : {m.in, m.comp, m.out})
    if (s) (void)hipStreamSynchronize(s);
  for (int i = 0; i < kPoolSlots; i++) {
    if (m.dev[i]) (void)hipFree(m.dev[i]);
    if (m.bounce[i]) (void)hipHostFree(m.bounce[i]);
    for (hipEvent_t e : {m.in_done[i], m.comp_done[i], m.out_done[i]})
      if (e) (void)hipEventDestroy(e);
    m.dev[i] = m.bounce[i] = nullptr;
  }
  if (m.shared) (void)hipFree(m.shared);
  if (m.status) (void)hipFree(m.status);
  if (m.flags) (void)hipHostFree(m.flags);
  for (auto& kv : m.key_copy) (void)hipFree(kv.second.dev);
  m.key_copy.clear();
  m.key_bytes = 0;
  m.set_relin.clear();
  m.set_galois.clear();
  m.relin_view.keys.clear();  // the views own nothing: KeysObj's destructor must not hand these to g_buffers
  m.galois_view.keys.clear();
  for (hipStream_t s : {m.in, m.comp, m.out})
    if (s) (void)hipStreamDestroy(s);
  m.in = m.comp = m.out = nullptr;
  m.eval.lower.clear();
  m.eval.ev.reset();
  m.eval.ctx.reset();
  m.relin_view.ctx.reset();
  m.galois_view.ctx.reset();
  m.ctx.reset();
}

bool grow_device(u64** p, size_t* cap, size_t words) {
  if (*cap >= words) return true;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipMalloc((void**)p, words * sizeof(u64)) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return false;
  }
  *cap = words;
  return true;
}

bool grow_pinned(void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return true;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipHostMalloc(p, bytes, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return false;
  }
  *cap = bytes;
  return true;
}

// The member's copies of `need` (a device-to-device copy on the same device, a peer copy across devices), made on first use
// and kept while the key buffer lives; copies of buffers that no longer live are dropped first.  With a bound (bytes, 0 = none)
// the least recently used copies that `need` does not name are dropped until `need` fits -- after the compute stream has
// drained, so no chunk in flight still reads them; a working set above the bound is E_OUTOFMEMORY.  `wait`: the copies have
// landed on return (otherwise they are ordered before whatever is launched on `s` next).
long member_stage_keys(PoolMember& m, const std::vector<PoolKey>& need, u64 bound, hipStream_t s, bool wait) {
  for (auto it = m.key_copy.begin(); it != m.key_copy.end();) {
    if (key_stamp_live(it->first)) {
      ++it;
      continue;
    }
    (void)hipFree(it->second.dev);
    m.key_bytes -= it->second.bytes;
    it = m.key_copy.erase(it);
  }
  const u64 now = ++m.key_tick;
  size_t working = 0, missing = 0;
  std::vector<const PoolKey*> todo;
  {
    std::set<u64> seen;
    for (const PoolKey& k : need) {
      if (!seen.insert(k.stamp).second) continue;
      const size_t bytes = k.words * sizeof(u64);
      working += bytes;
      auto it = m.key_copy.find(k.stamp);
      if (it != m.key_copy.end()) {
        it->second.tick = now;
        continue;
      }
      missing += bytes;
      todo.push_back(&k);
    }
  }
  if (bound && working > bound) {
    char msg[256];
    snprintf(msg, sizeof(msg),
             "the keys of one chunk take %llu bytes, the member's key cache is bounded at %llu bytes (lower hipbfv_Pool_SetChunk or raise "
             "hipbfv_Pool_SetKeyCacheBytes)",
             (unsigned long long)working, (unsigned long long)bound);
    return fail(HIPBFV_E_OUTOFMEMORY, msg);
  }
  if (bound && m.key_bytes + missing > bound) {
    if (hipStreamSynchronize(m.comp) != hipSuccess) return from_status(kHipError);
    while (m.key_bytes + missing > bound) {
      auto victim = m.key_copy.end();
      for (auto it = m.key_copy.begin(); it != m.key_copy.end(); ++it)
        if (it->second.tick != now && (victim == m.key_copy.end() || it->second.tick < victim->second.tick)) victim = it;
      if (victim == m.key_copy.end()) break;  // cannot happen: everything else is the working set, which fits
      (void)hipFree(victim->second.dev);
      m.key_bytes -= victim->second.bytes;
      m.key_evictions++;
      m.key_copy.erase(victim);
    }
  }
  for (const PoolKey* k : todo) {
    u64* d = nullptr;
    const size_t bytes = k->words * sizeof(u64);
    if (hipMalloc((void**)&d, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return from_status(kOutOfMemory);
    }
    const hipError_t e = k->src_device == m.device ? hipMemcpyAsync(d, k->src, bytes, hipMemcpyDeviceToDevice, s)
                                                   : hipMemcpyPeerAsync(d, m.device, k->src, k->src_device, bytes, s);
    if (e != hipSuccess || (wait && hipStreamSynchronize(s) != hipSuccess)) {
      (void)hipGetLastError();
      (void)hipFree(d);
      return from_status(kOutOfMemory);
    }
    m.key_copies++;
    m.key_bytes += bytes;
    m.key_copy[k->stamp] = PoolKeyCopy{d, bytes, now};
  }
  return HIPBFV_S_OK;
}

// The single-key calls: every buffer of the call's two handles, as the member's relin_view / galois_view
long member_keys(PoolMember& m, const std::vector<PoolKey>& relin, const std::vector<PoolKey>& galois, u64 bound) {
  std::vector<PoolKey> need(relin);
  need.insert(need.end(), galois.begin(), galois.end());
  m.relin_view.keys.clear();
  m.galois_view.keys.clear();
  if (long hr = member_stage_keys(m, need, bound, m.in, true)) return hr;
  for (const PoolKey& k : relin) m.relin_view.keys[k.index] = m.key_copy[k.stamp].dev;
  for (const PoolKey& k : galois) m.galois_view.keys[k.index] = m.key_copy[k.stamp].dev;
  return HIPBFV_S_OK;
}

// The key table of the chunk whose input sets name key_index[0, count): the member's copies of what the call needs of the
// chunk's distinct sets (copied on the compute stream, ahead of the chunk's kernels: no host synchronisation in the pipeline)
// behind handles of the member's context
long member_chunk_keys(PoolMember& m, const PoolSetKeys& all, const uint32_t* key_index, u64 count, u64 bound, PoolChunkKeys* ck) {
  pool_keyplan(key_index, count, &ck->sets, &ck->index);
  std::vector<PoolKey> need;
  for (uint32_t set : ck->sets) {
    need.insert(need.end(), all.relin[set].begin(), all.relin[set].end());
    need.insert(need.end(), all.galois[set].begin(), all.galois[set].end());
  }
  if (long hr = member_stage_keys(m, need, bound, m.comp, false)) return hr;
  const size_t nl = ck->sets.size();
  while (m.set_relin.size() < nl) {
    m.set_relin.emplace_back(new PoolKeyView());
    m.set_galois.emplace_back(new PoolKeyView());
    m.set_relin.back()->ctx = m.set_galois.back()->ctx = m.ctx;
  }
  ck->relin.assign(nl, nullptr);
  ck->galois.assign(nl, nullptr);
  for (size_t l = 0; l < nl; l++) {
    const uint32_t set = ck->sets[l];
    m.set_relin[l]->keys.clear();
    m.set_galois[l]->keys.clear();
    for (const PoolKey& k : all.relin[set]) m.set_relin[l]->keys[k.index] = m.key_copy[k.stamp].dev;
    for (const PoolKey& k : all.galois[set]) m.set_galois[l]->keys[k.index] = m.key_copy[k.stamp].dev;
    if (!all.relin[set].empty()) ck->relin[l] = m.set_relin[l].get();
    if (!all.galois[set].empty()) ck->galois[l] = m.set_galois[l].get();
  }
  return HIPBFV_S_OK;
}

// compute(chunk, device input pointers (shared inputs: the member's copy), device output pointers, sets, first global set)
using PoolCompute = std::function<long(u64, const std::vector<const u64*>&, const std::vector<u64*>&, u64, u64)>;

// Input sets [begin, end) of the call through the member's three-stream pipeline, `chunk` sets at a time: chunk j's
// host-to-device copies (in stream) overlap chunk j-1's compute and chunk j-2's device-to-host copies (out stream); the
// streams are ordered by events, and a slot's device memory is reused only after its previous chunk has been copied out.
long member_run(PoolMember& m, const std::vector<PoolIn>& ins, const std::vector<PoolOut>& outs, u64 begin, u64 end, u64 chunk,
                const PoolCompute& compute) {
  const u64 count = end - begin;
  if (!count) return HIPBFV_S_OK;
  chunk = std::min(chunk, count);  // buffers are sized to the chunk, never to more than the shard
  const u64 nch = (count + chunk - 1) / chunk;
  std::vector<size_t> in_off(ins.size(), 0), out_off(outs.size(), 0), shared_off(ins.size(), 0);
  size_t words = 0, shared_words = 0;
  bool pageable = false;
  for (size_t i = 0; i < ins.size(); i++) {
    if (!ins[i].stride) {
      shared_off[i] = shared_words;
      shared_words += ins[i].width;
      continue;
    }
    in_off[i] = words;
    words += ins[i].width * chunk;
    pageable |= !ins[i].pinned;
  }
  for (size_t k = 0; k < outs.size(); k++) {
    out_off[k] = words;
    words += outs[k].width * chunk;
    pageable |= !outs[k].pinned;
  }
  // slot memory: allocated once per pool, grown only when a call needs more than any call before it
  if (m.dev_words < words) {
    for (int i = 0; i < kPoolSlots; i++) {
      size_t cap = m.dev_words;
      if (!grow_device(&m.dev[i], &cap, words)) return from_status(kOutOfMemory);
    }
    m.dev_words = words;
  }
  if (pageable && m.bounce_words < words) {
    for (int i = 0; i < kPoolSlots; i++) {
      size_t cap = m.bounce_words * sizeof(u64);
      if (!grow_pinned((void**)&m.bounce[i], &cap, words * sizeof(u64))) return from_status(kOutOfMemory);
    }
    m.bounce_words = words;
  }
  if (shared_words && !grow_device(&m.shared, &m.shared_words, shared_words)) return from_status(kOutOfMemory);
  // shared plaintexts: once per call to each member (the in stream orders them before every chunk's inputs)
  for (size_t i = 0; i < ins.size(); i++)
    if (!ins[i].stride) {
      if (hipMemcpyAsync(m.shared + shared_off[i], ins[i].host, ins[i].width * sizeof(u64), hipMemcpyHostToDevice, m.in) != hipSuccess ||
          (!ins[i].pinned && hipStreamSynchronize(m.in) != hipSuccess))
        return from_status(kHipError);
    }

  auto sets_of = [&](u64 j) { return std::min<u64>(chunk, count - j * chunk); };
  auto stage_in = [&](u64 j) -> hipError_t {
    const int s = (int)(j % kPoolSlots);
    const u64 lo = begin + j * chunk, c = sets_of(j);
    hipError_t e = hipSuccess;
    if (j >= (u64)kPoolSlots) {
      if ((e = hipStreamWaitEvent(m.in, m.out_done[s], 0)) != hipSuccess) return e;  // the slot's last chunk has left the device
      if (pageable && (e = hipEventSynchronize(m.in_done[s])) != hipSuccess) return e;  // ... and its bounce copy has been read
    }
    for (size_t i = 0; i < ins.size(); i++) {
      const PoolIn& in = ins[i];
      if (!in.stride) continue;
      u64* d = m.dev[s] + in_off[i];
      const u64* src = in.host + lo * in.stride;
      const size_t bytes = c * in.width * sizeof(u64);
      if (in.pinned) {
        e = in.stride == in.width ? hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, m.in)
                                  : hipMemcpy2DAsync(d, in.width * sizeof(u64), src, in.stride * sizeof(u64), in.width * sizeof(u64), c,
                                                     hipMemcpyHostToDevice, m.in);
      } else {
        u64* h = m.bounce[s] + in_off[i];
        if (in.stride == in.width)
          std::memcpy(h, src, bytes);
        else
          for (u64 x = 0; x < c; x++) std::memcpy(h + x * in.width, src + x * in.stride, in.width * sizeof(u64));
        e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, m.in);
      }
      if (e != hipSuccess) return e;
    }
    return hipEventRecord(m.in_done[s], m.in);
  };
  auto drain_out = [&](u64 j) -> hipError_t {
    const int s = (int)(j % kPoolSlots);
    const u64 lo = begin + j * chunk, c = sets_of(j);
    hipError_t e = hipStreamWaitEvent(m.out, m.comp_done[s], 0);
    for (size_t k = 0; k < outs.size() && e == hipSuccess; k++) {
      u64* dst = outs[k].pinned ? outs[k].host + lo * outs[k].width : m.bounce[s] + out_off[k];
      e = hipMemcpyAsync(dst, m.dev[s] + out_off[k], c * outs[k].width * sizeof(u64), hipMemcpyDeviceToHost, m.out);
    }
    return e != hipSuccess ? e : hipEventRecord(m.out_done[s], m.out);
  };
  auto finish_out = [&](u64 j) -> hipError_t {  // pageable outputs: bounce -> caller once the chunk's copy has landed
    const int s = (int)(j % kPoolSlots);
    const u64 lo = begin + j * chunk, c = sets_of(j);
    bool any = false;
    for (const PoolOut& o : outs) any |= !o.pinned;
    if (!any) return hipSuccess;
    if (hipError_t e = hipEventSynchronize(m.out_done[s])) return e;
    for (size_t k = 0; k < outs.size(); k++)
      if (!outs[k].pinned) std::memcpy(outs[k].host + lo * outs[k].width, m.bounce[s] + out_off[k], c * outs[k].width * sizeof(u64));
    return hipSuccess;
  };
  auto drain_all = [&](long hr) {
    for (hipStream_t s : {m.in, m.comp, m.out}) (void)hipStreamSynchronize(s);
    return hr;
  };

  std::vector<const u64*> dins(ins.size());
  std::vector<u64*> douts(outs.size());
  if (stage_in(0) != hipSuccess || (nch > 1 && stage_in(1) != hipSuccess)) return drain_all(from_status(kHipError));
  for (u64 j = 0; j < nch; j++) {
    const int s = (int)(j % kPoolSlots);
    for (size_t i = 0; i < ins.size(); i++) dins[i] = ins[i].stride ? m.dev[s] + in_off[i] : m.shared + shared_off[i];
    for (size_t k = 0; k < outs.size(); k++) douts[k] = m.dev[s] + out_off[k];
    if (hipStreamWaitEvent(m.comp, m.in_done[s], 0) != hipSuccess) return drain_all(from_status(kHipError));
    if (long hr = compute(j, dins, douts, sets_of(j), begin + j * chunk)) return drain_all(hr);
    if (hipEventRecord(m.comp_done[s], m.comp) != hipSuccess || drain_out(j) != hipSuccess) return drain_all(from_status(kHipError));
    if (j + 2 < nch && stage_in(j + 2) != hipSuccess) return drain_all(from_status(kHipError));
    if (j >= 1 && finish_out(j - 1) != hipSuccess) return drain_all(from_status(kHipError));
  }
  if (finish_out(nch - 1) != hipSuccess) return drain_all(from_status(kHipError));
  return drain_all(hipStreamSynchronize(m.out) == hipSuccess ? HIPBFV_S_OK : from_status(kHipError));
}

// ---- on the calling thread ----
// Every member with a non-empty shard runs `job(member, begin, end)` on its worker; the first failure in set order is returned
// with its message as the calling thread's last error.
long pool_dispatch(PoolObj& p, u64 batch, const std::function<long(PoolMember&, u64, u64)>& job) {
  const u64 nm = p.members.size();
  std::vector<char> busy(nm, 0);
  for (u64 r = 0; r < nm; r++) {
    u64 lo, hi;
    pool_shard(batch, nm, r, &lo, &hi);
    if (lo == hi) continue;  // an empty shard launches nothing
    PoolMember* m = p.members[r].get();
    pool_submit(*m, [m, lo, hi, &job] { return job(*m, lo, hi); });
    busy[r] = 1;
  }
  long first = HIPBFV_S_OK;
  std::string msg;
  for (u64 r = 0; r < nm; r++) {
    if (!busy[r]) continue;
    std::string m;
    const long hr = pool_wait(*p.members[r], &m);
    if (hr != HIPBFV_S_OK && first == HIPBFV_S_OK) {
      first = hr;
      msg = m;
    }
  }
  if (first != HIPBFV_S_OK) tls_error = msg;
  return first;
}

// A key handle whose context has the pool's parameters (nullptr for NULL, a foreign object or other parameters)
KeysObj* pool_keyset(const PoolObj& p, void* handle) {
  KeysObj* k = as<KeysObj>(handle, kMagicKeys);
  return k && k->ctx && p.same_params(*k->ctx) ? k : nullptr;
}

// Key `index` of such a handle; false if it does not hold it
bool pool_key_of(KeysObj* k, u32 index, PoolKey* out) {
  auto kv = k->keys.find(index);
  auto st = k->stamps.find(index);
  if (kv == k->keys.end() || st == k->stamps.end()) return false;
  *out = PoolKey{index, st->second, kv->second, k->ctx->device(), k->ctx->key_words()};
  return true;
}

// The key buffers of a handle whose context has the pool's parameters (nothing for NULL, a foreign object or other parameters)
std::vector<PoolKey> pool_keys_of(const PoolObj& p, void* handle, bool relin_only) {
  std::vector<PoolKey> out;
  KeysObj* k = pool_keyset(p, handle);
  if (!k) return out;
  for (auto& kv : k->keys) {
    if (relin_only && kv.first != 0) continue;
    auto st = k->stamps.find(kv.first);
    if (st == k->stamps.end()) continue;
    out.push_back(PoolKey{kv.first, st->second, kv.second, k->ctx->device(), k->ctx->key_words()});
  }
  return out;
}

// ---- per-client key sets: on the calling thread ----
// What the call needs of one referenced set (its relinearisation and Galois handles, nullptr where the caller gave none):
// appends the buffers, false if the set lacks one
using PoolNeeds = std::function<bool(KeysObj*, KeysObj*, std::vector<PoolKey>*, std::vector<PoolKey>*)>;

// Pre-flight over the whole batch, before any member copies or launches anything: key_index in range, every referenced handle a
// key object of the pool's parameters holding what `needs` asks of it -- E_INVALIDARG naming the set's index in the caller's array
long pool_set_keys(const PoolObj& p, void* const* relin_sets, void* const* galois_sets, u64 num_sets, const uint32_t* key_index, u64 count,
                   const PoolNeeds& needs, PoolSetKeys* all) {
  for (u64 i = 0; i < count; i++)
    if (key_index[i] >= num_sets) {
      char msg[160];
      snprintf(msg, sizeof(msg), "key_index[%llu] names key set %u, but only %llu key sets were given", (unsigned long long)i, key_index[i],
               (unsigned long long)num_sets);
      return fail(HIPBFV_E_INVALIDARG, msg);
    }
  all->relin.assign(num_sets, {});
  all->galois.assign(num_sets, {});
  const std::vector<char> used = referenced_sets(key_index, count, num_sets);
  for (u64 k = 0; k < num_sets; k++) {
    if (!used[k]) continue;
    KeysObj* ko[2] = {nullptr, nullptr};
    int a = 0;
    for (void* const* arr : {relin_sets, galois_sets}) {
      void* h = arr ? arr[k] : nullptr;
      if (h && !(ko[a] = pool_keyset(p, h))) return no_key_in_set(k);  // not a key object, or of other parameters
      a++;
    }
    if (!needs(ko[0], ko[1], &all->relin[k], &all->galois[k])) return no_key_in_set(k);
  }
  return HIPBFV_S_OK;
}

// ---- the transparent-result watch of a call: `words` device status words, all read back after the last chunk (no small copy on
// the compute stream queues behind the out stream's large ones) ----
long member_watch_begin(PoolMember& m, u64 words) {
  if (m.status_cap < words) {
    if (m.status) (void)hipFree(m.status);
    m.status = nullptr;
    m.status_cap = 0;
    if (hipMalloc((void**)&m.status, words * sizeof(u32)) != hipSuccess) {
      (void)hipGetLastError();
      m.status = nullptr;
      return from_status(kOutOfMemory);
    }
    m.status_cap = words;
  }
  size_t cap = m.flag_cap;
  if (!grow_pinned((void**)&m.flags, &cap, words * sizeof(u32))) return from_status(kOutOfMemory);
  m.flag_cap = cap;
  if (hipMemsetAsync(m.status, 0xFF, words * sizeof(u32), m.comp) != hipSuccess) return from_status(kHipError);
  return HIPBFV_S_OK;
}

// m.flags[0, words) = the status words (0xFFFFFFFF: nothing transparent)
long member_watch_read(PoolMember& m, u64 words) {
  if (hipMemcpyAsync(m.flags, m.status, words * sizeof(u32), hipMemcpyDeviceToHost, m.comp) != hipSuccess || hipStreamSynchronize(m.comp) != hipSuccess)
    return from_status(kHipError);
  return HIPBFV_S_OK;
}

long pool_transparent(u64 set) {
  char msg[128];
  snprintf(msg, sizeof(msg), "result ciphertext is transparent (input set %llu of the batch)", (unsigned long long)set);
  return fail(HIPBFV_COR_E_INVALIDOPERATION, msg);
}

// A host operand of a pool call: pinned or pageable; false for device memory
bool pool_host_operand(const void* p, size_t bytes, bool* pinned) {
  const HostMem k = host_kind(p, bytes);
  *pinned = k == HostMem::kPinned;
  return k != HostMem::kDevice;
}

void pool_destroy(PoolObj* p) {
  for (auto& m : p->members) {
    if (!m->thread.joinable()) continue;
    PoolMember* mp = m.get();
    pool_submit(*mp, [mp] {
      member_release(*mp);
      return HIPBFV_S_OK;
    });
    std::string msg;
    (void)pool_wait(*mp, &msg);
    {
      std::lock_guard<std::mutex> g(mp->mu);
      mp->quit = true;
    }
    mp->cv.notify_all();
    mp->thread.join();
  }
  delete p;
}

}  // namespace
