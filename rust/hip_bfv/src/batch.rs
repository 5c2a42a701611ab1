//! The GPU batch executor seam: one graph node over `count` independent ciphertexts per call.
//!
//! `sunscreen_runtime/src/run.rs:160-341` issues one FFI call (and at least one allocation) per node per ciphertext.
//! Here a ciphertext batch is a device buffer `u64[count][size][K][N]` that never leaves HBM between nodes; operations
//! are asynchronous on the caller's HIP stream.  Transparent results (SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT,
//! `sunscreen/tests/features.rs:8-34`) are recorded on the device and surface at [`BatchEvaluator::check`] /
//! [`Program::run`], which is where this path synchronises.
use std::ffi::c_void;
use std::ptr::null_mut;

use crate::{bindgen, check, BFVEvaluator, GaloisKeys, RelinearizationKeys, Result, SecretKey};

/// A borrowed device buffer of `count` ciphertexts of `size` polynomials (memory is owned by the caller's allocator:
/// hipMalloc, a torch tensor, ...).  The library cannot check a device address: constructing one is the `unsafe` step, the
/// operations on a constructed batch are safe.
#[derive(Clone, Copy)]
pub struct DeviceBatch {
    ptr: *mut u64,
    size: u64,
    count: u64,
}

impl DeviceBatch {
    /// # Safety
    /// `ptr` must be a device address of at least `count * size * K * N` u64 words on the evaluator's device, valid (and,
    /// for outputs, not aliased by a concurrently running operation) until the stream work that uses it has completed.
    pub unsafe fn new(ptr: *mut u64, size: u64, count: u64) -> Self {
        Self { ptr, size, count }
    }
    pub fn ptr(&self) -> *mut u64 {
        self.ptr
    }
    pub fn size(&self) -> u64 {
        self.size
    }
    pub fn count(&self) -> u64 {
        self.count
    }
}

fn same_count(a: &DeviceBatch, b: &DeviceBatch) -> Result<()> {
    if a.count != b.count {
        return Err(crate::Error::InvalidArgument(format!("batches of {} and {} ciphertexts", a.count, b.count)));
    }
    Ok(())
}

/// A prepared second operand ([`BatchEvaluator::prepare`]): ciphertexts kept on the device, transformed once, usable by any number
/// of `*_shared` calls on any stream (the object carries an event).
pub struct Multiplicand {
    h: *mut c_void,
}

impl Multiplicand {
    pub fn count(&self) -> Result<u64> {
        let mut n = 0u64;
        check(unsafe { bindgen::hipbfv_Multiplicand_Count(self.h, &mut n) })?;
        Ok(n)
    }
    /// Device memory held: the copy of the ciphertexts and their transformed rows.
    pub fn bytes(&self) -> Result<u64> {
        let mut n = 0u64;
        check(unsafe { bindgen::hipbfv_Multiplicand_Bytes(self.h, &mut n) })?;
        Ok(n)
    }
}

impl Drop for Multiplicand {
    fn drop(&mut self) {
        unsafe { bindgen::hipbfv_Multiplicand_Destroy(self.h) };
    }
}

pub struct BatchEvaluator<'e> {
    eval: &'e BFVEvaluator,
    stream: *mut c_void,
}

impl<'e> BatchEvaluator<'e> {
    /// `stream`: a `hipStream_t` (null = the default stream).
    pub fn new(eval: &'e BFVEvaluator, stream: *mut c_void) -> Self {
        Self { eval, stream }
    }
    fn h(&self) -> *mut c_void {
        self.eval.get_handle()
    }

    pub fn multiply_relin(&self, a: DeviceBatch, b: DeviceBatch, rk: &RelinearizationKeys, out: DeviceBatch) -> Result<()> {
        same_count(&a, &b)?;
        same_count(&a, &out)?;
        check(unsafe { bindgen::hipbfv_batch_multiply_relin(self.h(), a.ptr, b.ptr, rk.get_handle(), out.ptr, a.count, self.stream) })
    }
    pub fn multiply(&self, a: DeviceBatch, b: DeviceBatch, out: DeviceBatch) -> Result<()> {
        same_count(&a, &b)?;
        same_count(&a, &out)?;
        check(unsafe { bindgen::hipbfv_batch_multiply(self.h(), a.ptr, a.size, b.ptr, b.size, out.ptr, a.count, self.stream) })
    }
    pub fn relinearize(&self, ct3: DeviceBatch, rk: &RelinearizationKeys, out: DeviceBatch) -> Result<()> {
        check(unsafe { bindgen::hipbfv_batch_relinearize(self.h(), ct3.ptr, rk.get_handle(), out.ptr, ct3.count, self.stream) })
    }
    pub fn rotate_rows(&self, a: DeviceBatch, steps: i32, gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        check(unsafe { bindgen::hipbfv_batch_rotate_rows(self.h(), a.ptr, steps, gk.get_handle(), out.ptr, a.count, self.stream) })
    }
    pub fn rotate_columns(&self, a: DeviceBatch, gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        check(unsafe { bindgen::hipbfv_batch_rotate_columns(self.h(), a.ptr, gk.get_handle(), out.ptr, a.count, self.stream) })
    }
    // ---- mixed-step rotation batches: item i by its own element / step in one key-switch pass (include/hipbfv.h) ----
    fn per_item_ok(len: usize, count: u64, what: &str) -> Result<()> {
        if len as u64 != count {
            return Err(crate::Error::InvalidArgument(format!("{} {} for {} items", len, what, count)));
        }
        Ok(())
    }
    pub fn apply_galois_items(&self, a: DeviceBatch, galois_elts: &[u32], gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        Self::per_item_ok(galois_elts.len(), a.count, "Galois elements")?;
        check(unsafe { bindgen::hipbfv_batch_apply_galois_items(self.h(), a.ptr, galois_elts.as_ptr(), gk.get_handle(), out.ptr, a.count, self.stream) })
    }
    pub fn rotate_rows_items(&self, a: DeviceBatch, steps: &[i32], gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        Self::per_item_ok(steps.len(), a.count, "steps")?;
        check(unsafe { bindgen::hipbfv_batch_rotate_rows_items(self.h(), a.ptr, steps.as_ptr(), gk.get_handle(), out.ptr, a.count, self.stream) })
    }
    // ---- sums of rotations: out[g] = sum_t rotate_rows(source of item g * terms + t, steps[t]) (include/hipbfv.h) ----
    // `a` holds the sources, `out` one ciphertext per group, terms = steps.len().  Item i reads source `src_index[i % src_index.len()]`;
    // `None` means source i (a.count == out.count * terms).  No in-place form.
    fn sum_sources_ok(a: &DeviceBatch, out: &DeviceBatch, terms: usize, src_index: Option<&[u32]>) -> Result<()> {
        let ok = terms > 0
            && match src_index {
                None => a.count == out.count * terms as u64,
                Some(idx) => !idx.is_empty() && idx.iter().all(|&i| (i as u64) < a.count),
            };
        if !ok {
            return Err(crate::Error::InvalidArgument(format!("{} sources for {} groups of {} terms", a.count, out.count, terms)));
        }
        Ok(())
    }
    pub fn rotate_rows_sum(&self, a: DeviceBatch, src_index: Option<&[u32]>, steps: &[i32], gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        Self::sum_sources_ok(&a, &out, steps.len(), src_index)?;
        let (ip, n) = src_index.map_or((std::ptr::null(), 0u64), |idx| (idx.as_ptr(), idx.len() as u64));
        check(unsafe {
            bindgen::hipbfv_batch_rotate_rows_sum(self.h(), a.ptr, a.count, ip, n, steps.as_ptr(), gk.get_handle(), out.ptr, out.count, steps.len() as u64, self.stream)
        })
    }
    pub fn apply_galois_sum(&self, a: DeviceBatch, src_index: Option<&[u32]>, galois_elts: &[u32], gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        Self::sum_sources_ok(&a, &out, galois_elts.len(), src_index)?;
        let (ip, n) = src_index.map_or((std::ptr::null(), 0u64), |idx| (idx.as_ptr(), idx.len() as u64));
        check(unsafe {
            bindgen::hipbfv_batch_apply_galois_sum(self.h(), a.ptr, a.count, ip, n, galois_elts.as_ptr(), gk.get_handle(), out.ptr, out.count, galois_elts.len() as u64, self.stream)
        })
    }
    // ---- weighted sums of rotations: out[g] = sum_t weights[t] (.) rotate_rows(source of item g * terms + t, steps[t]) ----
    // The two calls above with one weight per term, shared by every group (any i32): every word of residue row i of the finished term
    // times (weights[t] mod q_i), applied inside the key switch's last kernel just before the term is added (include/hipbfv.h).
    fn weights_ok(weights: &[i32], terms: usize) -> Result<()> {
        if weights.len() != terms {
            return Err(crate::Error::InvalidArgument(format!("{} weights for {} terms", weights.len(), terms)));
        }
        Ok(())
    }
    pub fn rotate_rows_sum_weighted(&self, a: DeviceBatch, src_index: Option<&[u32]>, steps: &[i32], weights: &[i32], gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        Self::sum_sources_ok(&a, &out, steps.len(), src_index)?;
        Self::weights_ok(weights, steps.len())?;
        let (ip, n) = src_index.map_or((std::ptr::null(), 0u64), |idx| (idx.as_ptr(), idx.len() as u64));
        check(unsafe {
            bindgen::hipbfv_batch_rotate_rows_sum_weighted(self.h(), a.ptr, a.count, ip, n, steps.as_ptr(), weights.as_ptr(), gk.get_handle(), out.ptr, out.count, steps.len() as u64, self.stream)
        })
    }
    pub fn apply_galois_sum_weighted(&self, a: DeviceBatch, src_index: Option<&[u32]>, galois_elts: &[u32], weights: &[i32], gk: &GaloisKeys, out: DeviceBatch) -> Result<()> {
        Self::sum_sources_ok(&a, &out, galois_elts.len(), src_index)?;
        Self::weights_ok(weights, galois_elts.len())?;
        let (ip, n) = src_index.map_or((std::ptr::null(), 0u64), |idx| (idx.as_ptr(), idx.len() as u64));
        check(unsafe {
            bindgen::hipbfv_batch_apply_galois_sum_weighted(self.h(), a.ptr, a.count, ip, n, galois_elts.as_ptr(), weights.as_ptr(), gk.get_handle(), out.ptr, out.count, galois_elts.len() as u64, self.stream)
        })
    }
    // ---- per-key batches ----
    // The reference hands the keys over with every call (`sunscreen_runtime/src/run.rs:100-105`: `relin_keys:
    // &Option<&RelinearizationKeys>`, `galois_keys: &Option<&GaloisKeys>`; `runtime.rs:310-327`): a server that batches the
    // calls of many clients holds one key set per client.  Item i uses `keys[key_index[i]]`; items need not be grouped by key.
    fn key_index_ok(key_index: &[u32], sets: usize, count: u64) -> Result<()> {
        if key_index.len() as u64 != count || key_index.iter().any(|&k| k as usize >= sets) {
            return Err(crate::Error::InvalidArgument(format!("{} key indices for {} items over {} key sets", key_index.len(), count, sets)));
        }
        Ok(())
    }
    pub fn multiply_relin_keys(&self, a: DeviceBatch, b: DeviceBatch, keys: &[&RelinearizationKeys], key_index: &[u32], out: DeviceBatch) -> Result<()> {
        same_count(&a, &b)?;
        same_count(&a, &out)?;
        Self::key_index_ok(key_index, keys.len(), a.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.get_handle()).collect();
        check(unsafe {
            bindgen::hipbfv_batch_multiply_relin_keys(self.h(), a.ptr, b.ptr, handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, a.count, self.stream)
        })
    }
    pub fn relinearize_keys(&self, ct3: DeviceBatch, keys: &[&RelinearizationKeys], key_index: &[u32], out: DeviceBatch) -> Result<()> {
        same_count(&ct3, &out)?;
        Self::key_index_ok(key_index, keys.len(), ct3.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.get_handle()).collect();
        check(unsafe {
            bindgen::hipbfv_batch_relinearize_keys(self.h(), ct3.ptr, handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, ct3.count, self.stream)
        })
    }
    // ---- sums of products with one relinearization per group (include/hipbfv.h) ----
    // `a`, `b`: `groups * terms` ciphertexts of size 2, group-major (`u64[groups][terms][2][K][N]`); `out`: one ciphertext per group.
    // The same batch as `a` and `b` sums squares.  No in-place form: the output may not overlap an operand.
    fn sum_shape_ok(a: &DeviceBatch, b: &DeviceBatch, terms: u64, out: &DeviceBatch) -> Result<()> {
        same_count(a, b)?;
        if terms == 0 || out.count.checked_mul(terms) != Some(a.count) {
            return Err(crate::Error::InvalidArgument(format!("{} terms of {} per group for {} groups", a.count, terms, out.count)));
        }
        Ok(())
    }
    pub fn multiply_sum(&self, a: DeviceBatch, b: DeviceBatch, terms: u64, out3: DeviceBatch) -> Result<()> {
        Self::sum_shape_ok(&a, &b, terms, &out3)?;
        check(unsafe { bindgen::hipbfv_batch_multiply_sum(self.h(), a.ptr, b.ptr, out3.ptr, out3.count, terms, self.stream) })
    }
    pub fn multiply_sum_relin(&self, a: DeviceBatch, b: DeviceBatch, terms: u64, rk: &RelinearizationKeys, out: DeviceBatch) -> Result<()> {
        Self::sum_shape_ok(&a, &b, terms, &out)?;
        check(unsafe { bindgen::hipbfv_batch_multiply_sum_relin(self.h(), a.ptr, b.ptr, rk.get_handle(), out.ptr, out.count, terms, self.stream) })
    }
    /// Group g is relinearised with `keys[key_index[g]]`; an entry no group names may be `None`.
    pub fn multiply_sum_relin_keys(&self, a: DeviceBatch, b: DeviceBatch, terms: u64, keys: &[Option<&RelinearizationKeys>], key_index: &[u32],
                                   out: DeviceBatch) -> Result<()> {
        Self::sum_shape_ok(&a, &b, terms, &out)?;
        Self::key_index_ok(key_index, keys.len(), out.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(std::ptr::null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_batch_multiply_sum_relin_keys(self.h(), a.ptr, b.ptr, handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, out.count, terms,
                                                          self.stream)
        })
    }
    /// `queries` queries against ONE pass over a transformed database.  `ctn`: `queries * cols` transformed size-2 ciphertexts
    /// (query-major), `pntt`: `rows * cols` transformed plaintexts as a batch of size 1 (row-major), `out`: `queries * rows` size-2
    /// ciphertexts -- what `multiply_sum_relin_keys` takes as `a` with `terms = rows`.  `out[q]` has the bits of the single-query product.
    pub fn dot_plain_ntt_queries(&self, ctn: DeviceBatch, queries: u64, pntt: DeviceBatch, rows: u64, out: DeviceBatch) -> Result<()> {
        let cols = if rows == 0 { 0 } else { pntt.count / rows };
        if ctn.size != 2 || out.size != 2 || pntt.size != 1 || cols == 0 || pntt.count != rows * cols || queries.checked_mul(cols) != Some(ctn.count)
            || queries.checked_mul(rows) != Some(out.count)
        {
            return Err(crate::Error::InvalidArgument(format!("{} query words, {} database words, {} outputs for {} queries and {} rows", ctn.count,
                                                             pntt.count, out.count, queries, rows)));
        }
        check(unsafe { bindgen::hipbfv_batch_dot_plain_ntt_queries(self.h(), ctn.ptr, queries, cols, pntt.ptr, rows, out.ptr, self.stream) })
    }
    // ---- weighted sums: out[g] = sum_t weights[t] * a[g][t] * b[g][t]; one weight per term, shared by every group (a weight multiplies
    // its term's noise by |w|) ----
    pub fn multiply_sum_weighted(&self, a: DeviceBatch, b: DeviceBatch, weights: &[i32], out3: DeviceBatch) -> Result<()> {
        let terms = weights.len() as u64;
        Self::sum_shape_ok(&a, &b, terms, &out3)?;
        check(unsafe { bindgen::hipbfv_batch_multiply_sum_weighted(self.h(), a.ptr, b.ptr, weights.as_ptr(), out3.ptr, out3.count, terms, self.stream) })
    }
    pub fn multiply_sum_weighted_relin(&self, a: DeviceBatch, b: DeviceBatch, weights: &[i32], rk: &RelinearizationKeys, out: DeviceBatch) -> Result<()> {
        let terms = weights.len() as u64;
        Self::sum_shape_ok(&a, &b, terms, &out)?;
        check(unsafe { bindgen::hipbfv_batch_multiply_sum_weighted_relin(self.h(), a.ptr, b.ptr, weights.as_ptr(), rk.get_handle(), out.ptr, out.count, terms, self.stream) })
    }
    pub fn multiply_sum_weighted_relin_keys(&self, a: DeviceBatch, b: DeviceBatch, weights: &[i32], keys: &[Option<&RelinearizationKeys>], key_index: &[u32],
                                            out: DeviceBatch) -> Result<()> {
        let terms = weights.len() as u64;
        Self::sum_shape_ok(&a, &b, terms, &out)?;
        Self::key_index_ok(key_index, keys.len(), out.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(std::ptr::null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_batch_multiply_sum_weighted_relin_keys(self.h(), a.ptr, b.ptr, weights.as_ptr(), handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr,
                                                                   out.count, terms, self.stream)
        })
    }
    // ---- prepared multiplicands: a shared second operand extended and transformed once (include/hipbfv.h) ----
    // Item i multiplies `a[i]` by prepared ciphertext `b_index[i % b_index.len()]`; in the sum forms i = g * terms + t.
    /// Copies the size-2 ciphertexts of `ct` and, where the parameter set has a split multiply, transforms them once.
    pub fn prepare(&self, ct: DeviceBatch) -> Result<Multiplicand> {
        let mut h: *mut c_void = null_mut();
        check(unsafe { bindgen::hipbfv_Multiplicand_Create(self.h(), ct.ptr, ct.count, self.stream, &mut h) })?;
        Ok(Multiplicand { h })
    }
    pub fn multiply_shared(&self, a: DeviceBatch, m: &Multiplicand, b_index: &[u32], out3: DeviceBatch) -> Result<()> {
        same_count(&a, &out3)?;
        check(unsafe { bindgen::hipbfv_batch_multiply_shared(self.h(), a.ptr, m.h, b_index.as_ptr(), b_index.len() as u64, out3.ptr, a.count, self.stream) })
    }
    /// `out` may be exactly `a`.
    pub fn multiply_relin_shared(&self, a: DeviceBatch, m: &Multiplicand, b_index: &[u32], rk: &RelinearizationKeys, out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_relin_shared(self.h(), a.ptr, m.h, b_index.as_ptr(), b_index.len() as u64, rk.get_handle(), out.ptr, a.count, self.stream)
        })
    }
    pub fn multiply_sum_shared(&self, a: DeviceBatch, m: &Multiplicand, b_index: &[u32], terms: u64, out3: DeviceBatch) -> Result<()> {
        Self::sum_shape_ok(&a, &a, terms, &out3)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_sum_shared(self.h(), a.ptr, m.h, b_index.as_ptr(), b_index.len() as u64, out3.ptr, out3.count, terms, self.stream)
        })
    }
    pub fn multiply_sum_relin_shared(&self, a: DeviceBatch, m: &Multiplicand, b_index: &[u32], terms: u64, rk: &RelinearizationKeys, out: DeviceBatch) -> Result<()> {
        Self::sum_shape_ok(&a, &a, terms, &out)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_sum_relin_shared(self.h(), a.ptr, m.h, b_index.as_ptr(), b_index.len() as u64, rk.get_handle(), out.ptr, out.count, terms,
                                                            self.stream)
        })
    }
    // ---- products of two prepared operands: no head, one middle kernel over both operands' rows (include/hipbfv.h) ----
    // Item i multiplies prepared ciphertext `a_index[i % L]` of `ma` by `b_index[i % L]` of `mb`, L = a_index.len() = b_index.len();
    // in the sum forms i = g * terms + t.  `ma` may be `mb`.
    fn pair_index_ok(a_index: &[u32], b_index: &[u32]) -> Result<()> {
        if a_index.len() != b_index.len() {
            return Err(crate::Error::InvalidArgument(format!("{} a indices and {} b indices", a_index.len(), b_index.len())));
        }
        Ok(())
    }
    pub fn multiply_prepared(&self, ma: &Multiplicand, a_index: &[u32], mb: &Multiplicand, b_index: &[u32], out3: DeviceBatch) -> Result<()> {
        Self::pair_index_ok(a_index, b_index)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_prepared(self.h(), ma.h, a_index.as_ptr(), mb.h, b_index.as_ptr(), a_index.len() as u64, out3.ptr, out3.count, self.stream)
        })
    }
    pub fn multiply_relin_prepared(&self, ma: &Multiplicand, a_index: &[u32], mb: &Multiplicand, b_index: &[u32], rk: &RelinearizationKeys,
                                   out: DeviceBatch) -> Result<()> {
        Self::pair_index_ok(a_index, b_index)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_relin_prepared(self.h(), ma.h, a_index.as_ptr(), mb.h, b_index.as_ptr(), a_index.len() as u64, rk.get_handle(), out.ptr,
                                                          out.count, self.stream)
        })
    }
    pub fn multiply_sum_prepared(&self, ma: &Multiplicand, a_index: &[u32], mb: &Multiplicand, b_index: &[u32], terms: u64, out3: DeviceBatch) -> Result<()> {
        Self::pair_index_ok(a_index, b_index)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_sum_prepared(self.h(), ma.h, a_index.as_ptr(), mb.h, b_index.as_ptr(), a_index.len() as u64, out3.ptr, out3.count, terms,
                                                        self.stream)
        })
    }
    pub fn multiply_sum_relin_prepared(&self, ma: &Multiplicand, a_index: &[u32], mb: &Multiplicand, b_index: &[u32], terms: u64, rk: &RelinearizationKeys,
                                       out: DeviceBatch) -> Result<()> {
        Self::pair_index_ok(a_index, b_index)?;
        check(unsafe {
            bindgen::hipbfv_batch_multiply_sum_relin_prepared(self.h(), ma.h, a_index.as_ptr(), mb.h, b_index.as_ptr(), a_index.len() as u64, rk.get_handle(),
                                                              out.ptr, out.count, terms, self.stream)
        })
    }
    /// The index tables of C = A B over prepared operands, A row-major m x k and B row-major k x n: item (i * n + j) * k + t multiplies
    /// A[i][t] (prepared ciphertext i * k + t) by B[t][j] (prepared ciphertext t * n + j); groups = m * n, terms = k.
    pub fn matrix_product_index(m: u32, k: u32, n: u32) -> (Vec<u32>, Vec<u32>) {
        let mut a_index = Vec::with_capacity((m * n * k) as usize);
        let mut b_index = Vec::with_capacity((m * n * k) as usize);
        for i in 0..m {
            for j in 0..n {
                for t in 0..k {
                    a_index.push(i * k + t);
                    b_index.push(t * n + j);
                }
            }
        }
        (a_index, b_index)
    }
    /// C = A B, `out` = m * n ciphertexts row-major: size 2 with one key switch per entry when `rk` is given, size-3 sums otherwise.
    pub fn matrix_product(&self, ma: &Multiplicand, mb: &Multiplicand, m: u32, k: u32, n: u32, rk: Option<&RelinearizationKeys>, out: DeviceBatch) -> Result<()> {
        let (a_index, b_index) = Self::matrix_product_index(m, k, n);
        match rk {
            Some(rk) => self.multiply_sum_relin_prepared(ma, &a_index, mb, &b_index, k as u64, rk, out),
            None => self.multiply_sum_prepared(ma, &a_index, mb, &b_index, k as u64, out),
        }
    }
    pub fn rotate_rows_keys(&self, a: DeviceBatch, steps: i32, keys: &[&GaloisKeys], key_index: &[u32], out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        Self::key_index_ok(key_index, keys.len(), a.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.get_handle()).collect();
        check(unsafe {
            bindgen::hipbfv_batch_rotate_rows_keys(self.h(), a.ptr, steps, handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, a.count, self.stream)
        })
    }
    pub fn rotate_columns_keys(&self, a: DeviceBatch, keys: &[&GaloisKeys], key_index: &[u32], out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        Self::key_index_ok(key_index, keys.len(), a.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.get_handle()).collect();
        check(unsafe {
            bindgen::hipbfv_batch_rotate_columns_keys(self.h(), a.ptr, handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, a.count, self.stream)
        })
    }
    // ---- mixed-step rotation batches with one key set per client: item i by its own element / step through `keys[key_index[i]]`;
    // an entry of `keys` that no rotating item names may be `None` ----
    pub fn apply_galois_items_keys(&self, a: DeviceBatch, galois_elts: &[u32], keys: &[Option<&GaloisKeys>], key_index: &[u32], out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        Self::per_item_ok(galois_elts.len(), a.count, "Galois elements")?;
        Self::key_index_ok(key_index, keys.len(), a.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(std::ptr::null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_batch_apply_galois_items_keys(self.h(), a.ptr, galois_elts.as_ptr(), handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, a.count, self.stream)
        })
    }
    pub fn rotate_rows_items_keys(&self, a: DeviceBatch, steps: &[i32], keys: &[Option<&GaloisKeys>], key_index: &[u32], out: DeviceBatch) -> Result<()> {
        same_count(&a, &out)?;
        Self::per_item_ok(steps.len(), a.count, "steps")?;
        Self::key_index_ok(key_index, keys.len(), a.count)?;
        let handles: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(std::ptr::null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_batch_rotate_rows_items_keys(self.h(), a.ptr, steps.as_ptr(), handles.as_ptr(), handles.len() as u64, key_index.as_ptr(), out.ptr, a.count, self.stream)
        })
    }
    pub fn add(&self, a: DeviceBatch, b: DeviceBatch, out: DeviceBatch) -> Result<()> {
        same_count(&a, &b)?;
        same_count(&a, &out)?;
        check(unsafe { bindgen::hipbfv_batch_add(self.h(), a.ptr, b.ptr, out.ptr, a.size, a.count, self.stream) })
    }
    pub fn sub(&self, a: DeviceBatch, b: DeviceBatch, out: DeviceBatch) -> Result<()> {
        same_count(&a, &b)?;
        same_count(&a, &out)?;
        check(unsafe { bindgen::hipbfv_batch_sub(self.h(), a.ptr, b.ptr, out.ptr, a.size, a.count, self.stream) })
    }
    pub fn negate(&self, a: DeviceBatch, out: DeviceBatch) -> Result<()> {
        check(unsafe { bindgen::hipbfv_batch_negate(self.h(), a.ptr, out.ptr, a.size, a.count, self.stream) })
    }
    /// Lift `count` coefficient-form plaintexts (`u64[count][N]`, stride `plain_stride` words) to the data primes and transform
    /// them: `pntt` = `u64[count][K][N]`, the operand `Input::PlaintextsNtt` takes.  An all-zero plaintext has no transformed
    /// form -- SEAL refuses every product with it (`sunscreen/tests/features.rs:8-34`) and the consumers cannot see it any
    /// more -- so this call ends with [`BatchEvaluator::check`] and fails with the index of the first one.
    ///
    /// # Safety
    /// `plain` and `pntt` must be device addresses of `count` plaintexts / `count * K * N` words on the evaluator's device.
    pub unsafe fn plain_to_ntt(&self, plain: *const u64, plain_stride: u64, pntt: *mut u64, count: u64) -> Result<()> {
        check(bindgen::hipbfv_batch_plain_to_ntt(self.h(), plain, plain_stride, pntt, count, self.stream))?;
        self.check()
    }
    /// `Decryptor::invariant_noise_budget` per item, on the device: `budget` = `i32[count]`, `noise` (optional) = the fork's
    /// `invariant_noise` as `f64[count]`.  `Runtime::measure_noise_budget` is the minimum of a value's budgets.  No output may
    /// overlap `ct` or another output.  Asynchronous: read `budget` after the stream work has completed.
    ///
    /// # Safety
    /// `budget` (and `noise`) must be device addresses of `ct.count()` entries on the evaluator's device.
    pub unsafe fn noise_budget(&self, ct: DeviceBatch, sk: &SecretKey, budget: *mut i32, noise: *mut f64) -> Result<()> {
        check(bindgen::hipbfv_batch_noise_budget(self.h(), ct.ptr, ct.size as u32, sk.get_handle(), budget, noise, ct.count, self.stream))
    }
    /// `hipbfv_batch_decrypt` and [`BatchEvaluator::noise_budget`] from one phase computation: `plain` = `u64[count][N]`,
    /// `budget` = `i32[count]`.  An item with budget 0 decrypted to garbage: `Runtime::decrypt` returns `Error::TooMuchNoise`.
    ///
    /// # Safety
    /// `plain` and `budget` must be device addresses of `ct.count()` plaintexts / entries on the evaluator's device.
    pub unsafe fn decrypt_checked(&self, ct: DeviceBatch, sk: &SecretKey, plain: *mut u64, budget: *mut i32) -> Result<()> {
        check(bindgen::hipbfv_batch_decrypt_checked(self.h(), ct.ptr, ct.size as u32, sk.get_handle(), plain, budget, ct.count, self.stream))
    }
    /// Synchronise the stream; `Err(InternalError(COR_E_INVALIDOPERATION, ..))` if any operation since the last call
    /// produced a transparent ciphertext.
    pub fn check(&self) -> Result<()> {
        let mut first = 0u64;
        check(unsafe { bindgen::hipbfv_batch_status(self.h(), &mut first, self.stream) })
    }
}

/// A compiled `FheProgram` graph (serde JSON of `sunscreen_fhe_program::FheProgram`, or built node by node) executed over
/// a batch of independent input sets: the replacement of `run_program_unchecked` (`run.rs:100-357`).
pub struct Program {
    handle: *mut c_void,
}
unsafe impl Sync for Program {}
unsafe impl Send for Program {}

pub enum Input {
    /// `u64[batch][2][K][N]` on the device
    Ciphertexts(*const u64),
    /// per-item plaintexts `u64[batch][N]` (stride N) or one shared `u64[N]` (stride 0), coefficient form, on the device
    Plaintexts { ptr: *const u64, stride: u64 },
    /// plaintexts already in transform form, `u64[batch][K][N]` (stride K*N) or shared (stride 0): the output of
    /// `hipbfv_batch_plain_to_ntt` -- a server's static database (examples/pir) is transformed once, not per query
    PlaintextsNtt { ptr: *const u64, stride: u64 },
}

impl Program {
    pub fn get_handle(&self) -> *mut c_void {
        self.handle
    }

    pub fn from_json(json: &str) -> Result<Self> {
        let mut handle = null_mut();
        check(unsafe { bindgen::hipbfv_Program_Create(&mut handle) })?;
        let p = Self { handle };
        check(unsafe { bindgen::hipbfv_Program_LoadJson(p.handle, json.as_ptr() as *const _, json.len() as u64) })?;
        Ok(p)
    }

    /// One output buffer `u64[batch][2][K][N]` per `OutputCiphertext` node, in node order.
    ///
    /// # Safety
    /// Every pointer in `inputs` and `outputs` must be a device address of the size its kind implies for `batch` items on
    /// the evaluator's device, valid until `stream` has drained (this call synchronises it before returning).
    pub unsafe fn run(
        &self, eval: &BFVEvaluator, batch: u64, inputs: &[Input], rk: Option<&RelinearizationKeys>, gk: Option<&GaloisKeys>,
        outputs: &[*mut u64], stream: *mut c_void,
    ) -> Result<()> {
        let kinds: Vec<u32> = inputs.iter().map(|i| match i { Input::Ciphertexts(_) => 0, Input::Plaintexts { .. } => 1, Input::PlaintextsNtt { .. } => 2 }).collect();
        let ptrs: Vec<*const u64> = inputs
            .iter()
            .map(|i| match i { Input::Ciphertexts(p) => *p, Input::Plaintexts { ptr, .. } | Input::PlaintextsNtt { ptr, .. } => *ptr })
            .collect();
        let strides: Vec<u64> = inputs
            .iter()
            .map(|i| match i { Input::Ciphertexts(_) => 0, Input::Plaintexts { stride, .. } | Input::PlaintextsNtt { stride, .. } => *stride })
            .collect();
        check(bindgen::hipbfv_Program_Run(
            self.handle, eval.get_handle(), batch, inputs.len() as u64, kinds.as_ptr(), ptrs.as_ptr(), strides.as_ptr(),
            rk.map_or(null_mut(), |k| k.get_handle()), gk.map_or(null_mut(), |k| k.get_handle()),
            outputs.len() as u64, outputs.as_ptr(), stream,
        ))
    }
}

impl Program {
    /// [`Program::run`] for a batch whose input sets belong to several clients: input set i runs with `rk[key_index[i]]`,
    /// `gk[key_index[i]]` (an entry may be `None` when the program needs no such key) -- the reference's per-call keys
    /// (`run.rs:100-105`) kept per input set.
    ///
    /// # Safety
    /// As for [`Program::run`].
    pub unsafe fn run_keys(
        &self, eval: &BFVEvaluator, batch: u64, inputs: &[Input], rk: &[Option<&RelinearizationKeys>], gk: &[Option<&GaloisKeys>],
        key_index: &[u32], outputs: &[*mut u64], stream: *mut c_void,
    ) -> Result<()> {
        let sets = rk.len().max(gk.len());
        if key_index.len() as u64 != batch || key_index.iter().any(|&k| k as usize >= sets) {
            return Err(crate::Error::InvalidArgument(format!("{} key indices for {} input sets over {} key sets", key_index.len(), batch, sets)));
        }
        let kinds: Vec<u32> = inputs.iter().map(|i| match i { Input::Ciphertexts(_) => 0, Input::Plaintexts { .. } => 1, Input::PlaintextsNtt { .. } => 2 }).collect();
        let ptrs: Vec<*const u64> = inputs
            .iter()
            .map(|i| match i { Input::Ciphertexts(p) => *p, Input::Plaintexts { ptr, .. } | Input::PlaintextsNtt { ptr, .. } => *ptr })
            .collect();
        let strides: Vec<u64> = inputs
            .iter()
            .map(|i| match i { Input::Ciphertexts(_) => 0, Input::Plaintexts { stride, .. } | Input::PlaintextsNtt { stride, .. } => *stride })
            .collect();
        let rks: Vec<*mut c_void> = (0..sets).map(|i| rk.get(i).copied().flatten().map_or(null_mut(), |k| k.get_handle())).collect();
        let gks: Vec<*mut c_void> = (0..sets).map(|i| gk.get(i).copied().flatten().map_or(null_mut(), |k| k.get_handle())).collect();
        check(bindgen::hipbfv_Program_RunKeys(
            self.handle, eval.get_handle(), batch, inputs.len() as u64, kinds.as_ptr(), ptrs.as_ptr(), strides.as_ptr(),
            sets as u64, rks.as_ptr(), gks.as_ptr(), key_index.as_ptr(), outputs.len() as u64, outputs.as_ptr(), stream,
        ))
    }
}

impl Drop for Program {
    fn drop(&mut self) {
        check(unsafe { bindgen::hipbfv_Program_Destroy(self.handle) }).expect("hipbfv_Program_Destroy");
    }
}
