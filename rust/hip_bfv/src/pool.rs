//! A pool of devices for host-resident batches: what `Runtime::run` hands over when its ciphertexts arrive from the network.
//!
//! Every member is one GPU with its own context, evaluator, streams and worker thread (`hipbfv_Pool_*`, include/hipbfv.h
//! "Device pool").  A call splits the batch into contiguous shards, one per member, and returns when every output is in host
//! memory; each member overlaps its host-to-device copies, its compute and its device-to-host copies.  Input set i gives
//! exactly the bits of the single-device call on input set i.  Host slices may be pinned or pageable.
//!
//! The `_keys` calls serve a batch whose input sets belong to several clients: input set i uses key set `key_index[i]`, in any
//! order, and a member copies only the keys its own shard names and the call needs ([`DevicePool::set_key_cache_bytes`] bounds
//! what it keeps).
use std::ffi::c_void;
use std::ptr::null_mut;

use crate::batch::Program;
use crate::{bindgen, check, Context, Error, GaloisKeys, RelinearizationKeys, Result};

pub struct DevicePool {
    handle: *mut c_void,
    ct_words: usize,
    n: usize,
}
// calls on one pool are serialised by the library; calls on different pools run concurrently
unsafe impl Sync for DevicePool {}
unsafe impl Send for DevicePool {}

/// One argument of [`DevicePool::run`], in host memory.
pub enum HostInput<'a> {
    /// `u64[batch][2][K][N]`
    Ciphertexts(&'a [u64]),
    /// per-set plaintexts `u64[batch][N]` in coefficient form
    Plaintexts(&'a [u64]),
    /// one plaintext `u64[N]` shared by every input set (sent to each member once per call)
    SharedPlaintext(&'a [u64]),
}

impl DevicePool {
    /// Members on `devices` (an ordinal may repeat: several members on one GPU), each with a context of `context`'s parameters.
    pub fn new(context: &Context, devices: &[i32]) -> Result<Self> {
        let (n, k, _, _) = context.info()?;
        let mut handle = null_mut();
        check(unsafe { bindgen::hipbfv_Pool_Create(context.get_handle(), devices.as_ptr(), devices.len() as u32, &mut handle) })?;
        Ok(Self { handle, ct_words: (2 * k * n) as usize, n: n as usize })
    }

    pub fn get_handle(&self) -> *mut c_void {
        self.handle
    }

    /// Input sets per pipeline chunk per member; 0 = the library's choice.
    pub fn set_chunk(&self, sets_per_chunk: u64) -> Result<()> {
        check(unsafe { bindgen::hipbfv_Pool_SetChunk(self.handle, sets_per_chunk) })
    }

    /// Bound, per member, on the bytes of key copies it keeps (least recently used copies go first); 0 = no bound (the default).
    pub fn set_key_cache_bytes(&self, bytes: u64) -> Result<()> {
        check(unsafe { bindgen::hipbfv_Pool_SetKeyCacheBytes(self.handle, bytes) })
    }

    /// One line per member: device, chunk, key copies made so far, buffer sizes, bytes of key copies held, copies dropped.
    pub fn describe(&self) -> Result<String> {
        let mut needed = 0u64;
        check(unsafe { bindgen::hipbfv_Pool_Describe(self.handle, null_mut(), 0, &mut needed) })?;
        let mut buf = vec![0u8; needed as usize];
        check(unsafe { bindgen::hipbfv_Pool_Describe(self.handle, buf.as_mut_ptr() as *mut _, needed, &mut needed) })?;
        let end = buf.iter().position(|&b| b == 0).unwrap_or(buf.len());
        Ok(String::from_utf8_lossy(&buf[..end]).into_owned())
    }

    /// `out = relinearize(a * b)` for every input set; `a`, `b` and `out` hold `u64[count][2][K][N]`.
    pub fn multiply_relin(&self, a: &[u64], b: &[u64], rk: &RelinearizationKeys, out: &mut [u64]) -> Result<()> {
        if a.len() != b.len() || a.len() != out.len() || a.len() % self.ct_words != 0 {
            return Err(Error::InvalidArgument(format!("slices of {}, {} and {} words for ciphertexts of {}", a.len(), b.len(), out.len(), self.ct_words)));
        }
        let count = (a.len() / self.ct_words) as u64;
        check(unsafe { bindgen::hipbfv_Pool_MultiplyRelin(self.handle, a.as_ptr(), b.as_ptr(), rk.get_handle(), out.as_mut_ptr(), count) })
    }

    fn count_of(&self, key_index: &[u32], slices: &[usize]) -> Result<u64> {
        let count = key_index.len();
        if slices.iter().any(|&len| len != count * self.ct_words) {
            return Err(Error::InvalidArgument(format!("slices of {:?} words for {} ciphertexts of {}", slices, count, self.ct_words)));
        }
        Ok(count as u64)
    }

    /// `out[i] = relinearize(a[i] * b[i])` with `keys[key_index[i]]`; an entry of `keys` that no input set names may be `None`.
    pub fn multiply_relin_keys(
        &self, a: &[u64], b: &[u64], keys: &[Option<&RelinearizationKeys>], key_index: &[u32], out: &mut [u64],
    ) -> Result<()> {
        let count = self.count_of(key_index, &[a.len(), b.len(), out.len()])?;
        let hs: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_Pool_MultiplyRelinKeys(self.handle, a.as_ptr(), b.as_ptr(), hs.as_ptr(), hs.len() as u64, key_index.as_ptr(), out.as_mut_ptr(), count)
        })
    }

    /// Rows rotated by `steps` with every input set's own Galois keys: a set that holds the key of `steps` uses it, a set with
    /// only the power-of-two keys takes the NAF chain, both in one call.
    pub fn rotate_rows_keys(&self, ct: &[u64], steps: i32, keys: &[Option<&GaloisKeys>], key_index: &[u32], out: &mut [u64]) -> Result<()> {
        let count = self.count_of(key_index, &[ct.len(), out.len()])?;
        let hs: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_Pool_RotateRowsKeys(self.handle, ct.as_ptr(), steps, hs.as_ptr(), hs.len() as u64, key_index.as_ptr(), out.as_mut_ptr(), count)
        })
    }

    /// Input set `i` rotated by `steps[i]` with `keys[key_index[i]]`: every (set, step) pair decides between the direct key and the
    /// NAF chain on its own, all in one call.
    pub fn rotate_rows_items_keys(&self, ct: &[u64], steps: &[i32], keys: &[Option<&GaloisKeys>], key_index: &[u32], out: &mut [u64]) -> Result<()> {
        let count = self.count_of(key_index, &[ct.len(), out.len()])?;
        if steps.len() as u64 != count {
            return Err(crate::Error::InvalidArgument(format!("{} steps for {} input sets", steps.len(), count)));
        }
        let hs: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_Pool_RotateRowsItemsKeys(self.handle, ct.as_ptr(), steps.as_ptr(), hs.as_ptr(), hs.len() as u64, key_index.as_ptr(), out.as_mut_ptr(), count)
        })
    }

    pub fn rotate_columns_keys(&self, ct: &[u64], keys: &[Option<&GaloisKeys>], key_index: &[u32], out: &mut [u64]) -> Result<()> {
        let count = self.count_of(key_index, &[ct.len(), out.len()])?;
        let hs: Vec<*mut c_void> = keys.iter().map(|k| k.map_or(null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            bindgen::hipbfv_Pool_RotateColumnsKeys(self.handle, ct.as_ptr(), hs.as_ptr(), hs.len() as u64, key_index.as_ptr(), out.as_mut_ptr(), count)
        })
    }

    /// A rotation batch with one shared key set.
    pub fn rotate_rows(&self, ct: &[u64], steps: i32, gk: &GaloisKeys, out: &mut [u64]) -> Result<()> {
        self.rotate_rows_keys(ct, steps, &[Some(gk)], &vec![0u32; ct.len() / self.ct_words], out)
    }

    pub fn rotate_columns(&self, ct: &[u64], gk: &GaloisKeys, out: &mut [u64]) -> Result<()> {
        self.rotate_columns_keys(ct, &[Some(gk)], &vec![0u32; ct.len() / self.ct_words], out)
    }

    /// [`Program::run`] over host memory: one `u64[batch][2][K][N]` output slice per `OutputCiphertext` node, in node order.
    pub fn run(
        &self, program: &Program, batch: u64, inputs: &[HostInput], rk: Option<&RelinearizationKeys>, gk: Option<&GaloisKeys>,
        outputs: &mut [&mut [u64]],
    ) -> Result<()> {
        self.run_keys(program, batch, inputs, &[rk], &[gk], None, outputs)
    }

    /// [`Program::run_keys`] over host memory: input set i runs with `rk[key_index[i]]`, `gk[key_index[i]]` (`key_index`
    /// `None`: the one key set of [`DevicePool::run`]).
    pub fn run_keys(
        &self, program: &Program, batch: u64, inputs: &[HostInput], rk: &[Option<&RelinearizationKeys>], gk: &[Option<&GaloisKeys>],
        key_index: Option<&[u32]>, outputs: &mut [&mut [u64]],
    ) -> Result<()> {
        let (ct, n, b) = (self.ct_words, self.n, batch as usize);
        let sets = rk.len().max(gk.len());
        if let Some(ki) = key_index {
            if ki.len() != b || sets == 0 {
                return Err(Error::InvalidArgument(format!("{} key indices for {} input sets over {} key sets", ki.len(), batch, sets)));
            }
        }
        for i in inputs {
            let (len, want) = match i {
                HostInput::Ciphertexts(s) => (s.len(), b * ct),
                HostInput::Plaintexts(s) => (s.len(), b * n),
                HostInput::SharedPlaintext(s) => (s.len(), n),
            };
            if len != want {
                return Err(Error::InvalidArgument(format!("an input of {} words where {} are needed", len, want)));
            }
        }
        if outputs.iter().any(|o| o.len() != b * ct) {
            return Err(Error::InvalidArgument(format!("every output needs {} words", b * ct)));
        }
        let kinds: Vec<u32> = inputs.iter().map(|i| match i { HostInput::Ciphertexts(_) => 0, _ => 1 }).collect();
        let ptrs: Vec<*const u64> = inputs
            .iter()
            .map(|i| match i { HostInput::Ciphertexts(s) | HostInput::Plaintexts(s) | HostInput::SharedPlaintext(s) => s.as_ptr() })
            .collect();
        let strides: Vec<u64> = inputs.iter().map(|i| match i { HostInput::Plaintexts(_) => n as u64, _ => 0 }).collect();
        let outs: Vec<*mut u64> = outputs.iter_mut().map(|o| o.as_mut_ptr()).collect();
        let rks: Vec<*mut c_void> = (0..sets).map(|i| rk.get(i).copied().flatten().map_or(null_mut(), |k| k.get_handle())).collect();
        let gks: Vec<*mut c_void> = (0..sets).map(|i| gk.get(i).copied().flatten().map_or(null_mut(), |k| k.get_handle())).collect();
        check(unsafe {
            match key_index {
                None => bindgen::hipbfv_Pool_ProgramRun(
                    self.handle, program.get_handle(), batch, inputs.len() as u64, kinds.as_ptr(), ptrs.as_ptr(), strides.as_ptr(),
                    rks.first().copied().unwrap_or(null_mut()), gks.first().copied().unwrap_or(null_mut()), outs.len() as u64, outs.as_ptr(),
                ),
                Some(ki) => bindgen::hipbfv_Pool_ProgramRunKeys(
                    self.handle, program.get_handle(), batch, inputs.len() as u64, kinds.as_ptr(), ptrs.as_ptr(), strides.as_ptr(),
                    sets as u64, rks.as_ptr(), gks.as_ptr(), ki.as_ptr(), outs.len() as u64, outs.as_ptr(),
                ),
            }
        })
    }
}

impl Drop for DevicePool {
    fn drop(&mut self) {
        check(unsafe { bindgen::hipbfv_Pool_Destroy(self.handle) }).expect("hipbfv_Pool_Destroy");
    }
}
