"""DevicePool: host-fed batches sharded over several GPUs in one process (hipbfv_Pool_*, include/hipbfv.h "Device pool").

Every member is one device with its own context (the parameters of `context`), evaluator, streams and worker thread; a call
splits the batch into contiguous shards (sunscreen_amd/dist.py:shard_range), and every member overlaps its host-to-device
copies, its compute and its device-to-host copies.  Inputs and outputs are HOST memory: numpy arrays or CPU tensors, pinned
(torch's pin_memory) or not.  Input set i gives exactly the bits of the single-device call on input set i.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from .seal import Context, GaloisKeys, RelinearizationKeys, _check


def _host(x):
    """(address, words, shape, keep-alive) of a host array: numpy (any integer dtype of 8 bytes) or a contiguous CPU tensor."""
    try:
        import torch
    except Exception:  # pragma: no cover - torch is a dependency of the package
        torch = None
    if torch is not None and isinstance(x, torch.Tensor):
        assert x.device.type == "cpu", "DevicePool takes host memory (numpy arrays or CPU tensors)"
        assert x.element_size() == 8 and x.is_contiguous(), (x.dtype, x.is_contiguous())
        return x.data_ptr(), x.numel(), tuple(x.shape), x
    a = np.ascontiguousarray(np.asarray(x))
    assert a.dtype.itemsize == 8 and a.dtype.kind in "iu", a.dtype
    return a.ctypes.data, a.size, a.shape, a


def _as_u64(x) -> np.ndarray:
    try:
        import torch

        if isinstance(x, torch.Tensor):
            return x.numpy().view(np.uint64)
    except Exception:  # pragma: no cover
        pass
    return x.view(np.uint64)


class DevicePool:
    """DevicePool(context, devices): members on `devices` (an ordinal may repeat: several members on one GPU)."""

    def __init__(self, context: Context, devices: Sequence[int] = (0,)):
        devices = list(devices)
        self._ctx = context
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check(_lib.load().hipbfv_Pool_Create(context.get_handle(), arr, len(devices), C.byref(self._h)))
        self.devices = devices
        self.n, self.K = context.poly_modulus_degree, context.K

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _lib.load().hipbfv_Pool_Destroy(h)
            self._h = C.c_void_p()

    def close(self) -> None:
        self.__del__()

    def get_handle(self) -> C.c_void_p:
        return self._h

    def set_chunk(self, sets_per_chunk: int) -> None:
        """Input sets per pipeline chunk per member; 0 = the library's choice."""
        _check(_lib.load().hipbfv_Pool_SetChunk(self._h, int(sets_per_chunk)))

    def set_key_cache_bytes(self, nbytes: int) -> None:
        """Bound, per member, on the bytes of key copies it keeps (least recently used copies go first); 0 = no bound."""
        _check(_lib.load().hipbfv_Pool_SetKeyCacheBytes(self._h, int(nbytes)))

    def describe(self) -> str:
        need = C.c_uint64()
        _check(_lib.load().hipbfv_Pool_Describe(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _check(_lib.load().hipbfv_Pool_Describe(self._h, buf, need.value, C.byref(need)))
        return buf.value.decode()

    def _out(self, out, batch):
        if out is None:
            out = np.empty((batch, 2, self.K, self.n), dtype=np.uint64)
        ptr, words, shape, keep = _host(out)
        assert keep is out, "an output must be a contiguous host array of 8-byte integers"
        assert words == batch * 2 * self.K * self.n, (shape, batch)
        return out, ptr

    def multiply_relin(self, a, b, relin_keys: RelinearizationKeys, out=None) -> np.ndarray:
        """relinearize(a * b) for every pair: a, b u64[batch][2][K][N] in host memory; returns the host array (or `out`)."""
        pa, wa, sa, ka = _host(a)
        pb, wb, sb, kb = _host(b)
        batch = sa[0] if len(sa) == 4 else 0
        assert len(sa) == 4 and tuple(sa) == tuple(sb) and tuple(sa[1:]) == (2, self.K, self.n), (sa, sb)
        out, po = self._out(out, batch)
        _check(_lib.load().hipbfv_Pool_MultiplyRelin(self._h, pa, pb, relin_keys.get_handle(), po, batch))
        return _as_u64(out)

    # ---- per-client key sets: input set i uses key_sets[key_index[i]]; a member copies only what its own chunks name ----
    @staticmethod
    def _key_sets(key_sets, key_index, count: int):
        # a None entry is a NULL handle: allowed for a set no input set names
        handles = (C.c_void_p * len(key_sets))(*[k.get_handle() if k is not None else None for k in key_sets])
        idx = np.ascontiguousarray(np.asarray(key_index, dtype=np.uint32))
        assert idx.shape == (count,), (idx.shape, count)
        return handles, len(key_sets), idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx

    def _one_ct(self, ct):
        ptr, _, shape, keep = _host(ct)
        assert len(shape) == 4 and tuple(shape[1:]) == (2, self.K, self.n), shape
        return ptr, shape[0], keep

    def multiply_relin_keys(self, a, b, key_sets: Sequence[RelinearizationKeys | None], key_index, out=None) -> np.ndarray:
        """relinearize(a * b) with key_sets[key_index[i]] for pair i (key_index: `batch` host integers, in any order)."""
        pa, batch, ka = self._one_ct(a)
        pb, batch_b, kb = self._one_ct(b)
        assert batch == batch_b, (batch, batch_b)
        out, po = self._out(out, batch)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, batch)
        _check(_lib.load().hipbfv_Pool_MultiplyRelinKeys(self._h, pa, pb, hs, n, ip, po, batch))
        return _as_u64(out)

    def rotate_rows_keys(self, ct, steps: int, key_sets: Sequence[GaloisKeys | None], key_index, out=None) -> np.ndarray:
        """Every ciphertext's rows rotated by `steps` with its own client's Galois keys: a set that holds the key of `steps` uses
        it, a set that holds only power-of-two keys takes the NAF chain, both in one call.  `out` may be `ct` itself."""
        pc, batch, kc = self._one_ct(ct)
        out, po = self._out(out, batch)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, batch)
        _check(_lib.load().hipbfv_Pool_RotateRowsKeys(self._h, pc, int(steps), hs, n, ip, po, batch))
        return _as_u64(out)

    def rotate_rows_items_keys(self, ct, steps, key_sets: Sequence[GaloisKeys | None], key_index, out=None) -> np.ndarray:
        """Ciphertext i rotated by steps[i] with key_sets[key_index[i]] (both `batch` host integers, in any order): every (set,
        step) pair decides on its own between a copy, the direct key and the NAF chain.  `out` may be `ct` itself."""
        pc, batch, kc = self._one_ct(ct)
        out, po = self._out(out, batch)
        st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
        assert st.shape == (batch,), (st.shape, batch)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, batch)
        _check(_lib.load().hipbfv_Pool_RotateRowsItemsKeys(self._h, pc, st.ctypes.data_as(C.POINTER(C.c_int32)), hs, n, ip, po, batch))
        return _as_u64(out)

    def rotate_columns_keys(self, ct, key_sets: Sequence[GaloisKeys | None], key_index, out=None) -> np.ndarray:
        pc, batch, kc = self._one_ct(ct)
        out, po = self._out(out, batch)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, batch)
        _check(_lib.load().hipbfv_Pool_RotateColumnsKeys(self._h, pc, hs, n, ip, po, batch))
        return _as_u64(out)

    def rotate_rows(self, ct, steps: int, galois_keys: GaloisKeys, out=None) -> np.ndarray:
        """A rotation batch with one shared key set (one key set, an all-zero key_index)."""
        return self.rotate_rows_keys(ct, steps, [galois_keys], np.zeros(_host(ct)[2][0], dtype=np.uint32), out)

    def rotate_columns(self, ct, galois_keys: GaloisKeys, out=None) -> np.ndarray:
        return self.rotate_columns_keys(ct, [galois_keys], np.zeros(_host(ct)[2][0], dtype=np.uint32), out)

    def run(self, program, inputs, relin_keys=None, galois_keys=None, outputs=None, key_index=None) -> list[np.ndarray]:
        """hipbfv_Program_Run's contract over host memory: inputs[i] is a ciphertext batch u64[batch][2][K][N], per-set
        plaintexts u64[batch][N] or one shared plaintext u64[N]; returns one host array u64[batch][2][K][N] per output.
        key_index (optional, `batch` host integers): one key set per client -- relin_keys / galois_keys are then SEQUENCES of key
        objects (an entry may be None) and input set i runs with relin_keys[key_index[i]], galois_keys[key_index[i]]."""
        hosts = [_host(x) for x in inputs]
        batch = None
        for _, _, shape, _ in hosts:
            if len(shape) == 4:
                batch = shape[0]
        assert batch is not None, "need at least one ciphertext argument"
        n_in = len(inputs)
        kinds = (C.c_uint32 * n_in)()
        ptrs = (C.c_void_p * n_in)()
        strides = (C.c_uint64 * n_in)()
        for i, (ptr, _, shape, _) in enumerate(hosts):
            if len(shape) == 4:
                assert shape == (batch, 2, self.K, self.n), shape
                kinds[i], strides[i] = 0, 0
            else:
                assert shape[-1] == self.n and (len(shape) == 1 or (len(shape) == 2 and shape[0] in (1, batch))), shape
                kinds[i] = 1
                strides[i] = 0 if len(shape) == 1 or shape[0] == 1 else self.n
            ptrs[i] = ptr
        n_out = program.num_outputs()
        if outputs is None:
            outputs = [None] * n_out
        assert len(outputs) == n_out
        outs = [self._out(o, batch) for o in outputs]
        optrs = (C.c_void_p * n_out)(*[p for _, p in outs])
        if key_index is not None:
            nsets = max(len(relin_keys) if relin_keys is not None else 0, len(galois_keys) if galois_keys is not None else 0)
            assert nsets > 0, "key_index needs sequences of key sets"
            rks = list(relin_keys) if relin_keys is not None else [None] * nsets
            gks = list(galois_keys) if galois_keys is not None else [None] * nsets
            assert len(rks) == len(gks) == nsets, (len(rks), len(gks))
            rh, _, ip, _keep = self._key_sets(rks, key_index, batch)
            gh, _, _, _ = self._key_sets(gks, key_index, batch)
            _check(_lib.load().hipbfv_Pool_ProgramRunKeys(self._h, program._h, batch, n_in, kinds, ptrs, strides, nsets, rh, gh, ip, n_out, optrs))
            return [_as_u64(o) for o, _ in outs]
        rk = relin_keys.get_handle() if relin_keys is not None else None
        gk = galois_keys.get_handle() if galois_keys is not None else None
        _check(_lib.load().hipbfv_Pool_ProgramRun(self._h, program._h, batch, n_in, kinds, ptrs, strides, rk, gk, n_out, optrs))
        return [_as_u64(o) for o, _ in outs]


def shard(batch: int, members: int, member: int) -> tuple[int, int]:
    """The library's split of a batch over pool members (host only; the rule of dist.shard_range)."""
    lo, hi = C.c_uint64(), C.c_uint64()
    _check(_lib.load().hipbfv_debug_pool_shard(batch, members, member, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def keyplan(key_index, num_key_sets: int, members: int, member: int, chunk: int, chunk_no: int) -> tuple[list[int], list[int]]:
    """The library's key table of one pipeline chunk (host only): the distinct key sets that chunk `chunk_no` of member
    `member`'s shard names, ascending, and the chunk's key_index remapped onto them."""
    idx = np.ascontiguousarray(np.asarray(key_index, dtype=np.uint32))
    local = (C.c_uint32 * max(1, num_key_sets))()
    remapped = (C.c_uint32 * max(1, chunk))()
    nl, nc = C.c_uint64(), C.c_uint64()
    _check(_lib.load().hipbfv_debug_pool_keyplan(idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size, num_key_sets, members, member, chunk,
                                                 chunk_no, local, C.byref(nl), remapped, C.byref(nc)))
    return list(local[: nl.value]), list(remapped[: nc.value])
