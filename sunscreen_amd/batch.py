"""GPU batch executor: Evaluator operations over device-resident batches of ciphertexts.

Replaces the reference's per-node dispatch (sunscreen_runtime/src/run.rs:160-341: one
`evaluator.<op>()` FFI call and at least one allocation per graph node per ciphertext) with one
sequence of kernel launches per operation over `count` independent ciphertexts.  Tensors are
`torch.int64` CUDA tensors holding uint64 bit patterns, shape [count, size, K, N]; PyTorch is used
only for device memory and streams -- all arithmetic happens in libhipbfv.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .seal import BFVEvaluator, Context, GaloisKeys, RelinearizationKeys, _check


def to_device(a: np.ndarray, device: str = "cuda:0") -> torch.Tensor:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _ptr(t: torch.Tensor):
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class BatchEvaluator:
    """`out=`: an output may be exactly one of the inputs (the same tensor) when it has that input's shape -- add(a, b, out=a),
    multiply_relin(a, a, out=a), rotate_rows(ct, s, gk, out=ct).  Any other overlap between an output and an input (a shifted
    view of the same storage, an output of another width such as multiply(a, b, out=a), relinearize(ct3, rk, out=ct3)) is
    refused with HipBfvError (InvalidArgument) before anything is launched (include/hipbfv.h, "Aliasing")."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._ev = BFVEvaluator(ctx)
        self._h = self._ev.get_handle()
        self.n, self.K, self.KK = ctx.poly_modulus_degree, ctx.K, ctx.KK

    def check(self) -> None:
        """Raise HipBfvError (COR_E_INVALIDOPERATION, as the reference's runtime does: sunscreen/tests/features.rs:8-34) if
        any batched operation since the last call produced a transparent ciphertext; synchronises the current stream.
        The operations themselves stay asynchronous: call this where the reference would have seen the error -- at the
        latest before results leave the device."""
        first = C.c_uint64()
        _check(_lib.load().hipbfv_batch_status(self._h, C.byref(first), _stream()))

    def set_transparent_check(self, enabled: bool) -> None:
        _check(_lib.load().hipbfv_set_batch_transparent_check(self._h, enabled))

    def set_chunk_ops(self, chunk: int) -> None:
        _check(_lib.load().hipbfv_set_chunk_ops(self._h, chunk))

    # ---- per-kernel HIP-event timing (bench.py) ----
    def profile(self, enabled: bool = True) -> None:
        _check(_lib.load().hipbfv_profile_enable(self._h, enabled))

    def profile_reset(self) -> None:
        _check(_lib.load().hipbfv_profile_reset(self._h))

    def profile_read(self) -> dict[str, dict]:
        L = _lib.load()
        cnt = C.c_uint32()
        _check(L.hipbfv_profile_kernel_count(C.byref(cnt)))
        out = {}
        for i in range(cnt.value):
            name = C.create_string_buffer(64)
            ms, launches, units = C.c_double(), C.c_uint64(), C.c_uint64()
            _check(L.hipbfv_profile_read(self._h, i, name, 64, C.byref(ms), C.byref(launches), C.byref(units)))
            if launches.value:
                out[name.value.decode()] = {"ms": ms.value, "launches": launches.value, "units": units.value}
        return out

    def _shape_ok(self, t: torch.Tensor, size=None):
        assert t.dim() == 4 and t.shape[2] == self.K and t.shape[3] == self.n, tuple(t.shape)
        if size is not None:
            assert t.shape[1] == size, tuple(t.shape)

    def _new(self, count: int, size: int, like: torch.Tensor) -> torch.Tensor:
        return torch.empty((count, size, self.K, self.n), dtype=torch.int64, device=like.device)

    # ---- a1 / a2 ----
    def multiply(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(a)
        self._shape_ok(b)
        count, sa, sb = a.shape[0], a.shape[1], b.shape[1]
        assert b.shape[0] == count
        out = out if out is not None else self._new(count, sa + sb - 1, a)
        _check(_lib.load().hipbfv_batch_multiply(self._h, _ptr(a), sa, _ptr(b), sb, _ptr(out), count, _stream()))
        return out

    def relinearize(self, ct3: torch.Tensor, rk: RelinearizationKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct3, 3)
        out = out if out is not None else self._new(ct3.shape[0], 2, ct3)
        _check(_lib.load().hipbfv_batch_relinearize(self._h, _ptr(ct3), rk.get_handle(), _ptr(out), ct3.shape[0], _stream()))
        return out

    def multiply_relin(self, a: torch.Tensor, b: torch.Tensor, rk: RelinearizationKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(a, 2)
        self._shape_ok(b, 2)
        assert a.shape[0] == b.shape[0]
        out = out if out is not None else self._new(a.shape[0], 2, a)
        _check(_lib.load().hipbfv_batch_multiply_relin(self._h, _ptr(a), _ptr(b), rk.get_handle(), _ptr(out), a.shape[0], _stream()))
        return out

    # ---- a3 ----
    def apply_galois(self, ct: torch.Tensor, galois_elt: int, gk: GaloisKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        _check(_lib.load().hipbfv_batch_apply_galois(self._h, _ptr(ct), galois_elt, gk.get_handle(), _ptr(out), ct.shape[0], _stream()))
        return out

    def rotate_rows(self, ct: torch.Tensor, steps: int, gk: GaloisKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        _check(_lib.load().hipbfv_batch_rotate_rows(self._h, _ptr(ct), steps, gk.get_handle(), _ptr(out), ct.shape[0], _stream()))
        return out

    def rotate_columns(self, ct: torch.Tensor, gk: GaloisKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        _check(_lib.load().hipbfv_batch_rotate_columns(self._h, _ptr(ct), gk.get_handle(), _ptr(out), ct.shape[0], _stream()))
        return out

    # ---- mixed-step rotation batches: item i by its own element / step, one key-switch pass (include/hipbfv.h) ----
    def apply_galois_items(self, ct: torch.Tensor, galois_elts, gk: GaloisKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        """Item i by galois_elts[i] (`count` host integers, odd and below 2 N; 1 copies the item)."""
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        elts = np.ascontiguousarray(np.asarray(galois_elts, dtype=np.uint32))
        assert elts.shape == (ct.shape[0],), (elts.shape, ct.shape[0])
        _check(_lib.load().hipbfv_batch_apply_galois_items(self._h, _ptr(ct), elts.ctypes.data_as(C.POINTER(C.c_uint32)), gk.get_handle(), _ptr(out),
                                                           ct.shape[0], _stream()))
        return out

    def rotate_rows_items(self, ct: torch.Tensor, steps, gk: GaloisKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        """Item i rotated by steps[i] (`count` host integers): the bits of rotate_rows(ct[i:i+1], steps[i], gk).  The steps whose
        own key gk holds share one launch sequence; step 0 copies; the others run their NAF chains, grouped by step."""
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
        assert st.shape == (ct.shape[0],), (st.shape, ct.shape[0])
        _check(_lib.load().hipbfv_batch_rotate_rows_items(self._h, _ptr(ct), st.ctypes.data_as(C.POINTER(C.c_int32)), gk.get_handle(), _ptr(out),
                                                          ct.shape[0], _stream()))
        return out

    # ---- sums of rotations: every term finished and added inside the key switch's last kernel (include/hipbfv.h) ----
    def _rotation_sum_args(self, ct: torch.Tensor, terms: int, groups, src_index, out):
        self._shape_ok(ct, 2)
        assert terms > 0, "a sum of rotations needs at least one term per group"
        if src_index is None:
            assert ct.shape[0] % terms == 0, (ct.shape[0], terms)
            groups = ct.shape[0] // terms if groups is None else groups
            assert groups * terms == ct.shape[0], (groups, terms, ct.shape[0])
            idx, ip, n = None, None, 0
        else:
            idx = np.ascontiguousarray(np.asarray(src_index, dtype=np.uint32))
            assert idx.ndim == 1 and idx.size > 0, idx.shape
            assert int(idx.max()) < ct.shape[0], (int(idx.max()), ct.shape[0])
            if groups is None:
                assert idx.size % terms == 0, (idx.size, terms)
                groups = idx.size // terms
            ip, n = idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size
        if out is None:
            out = self._new(groups, 2, ct)
        self._shape_ok(out, 2)
        assert out.shape[0] == groups, (out.shape[0], groups)
        return groups, ip, n, out, idx

    def rotate_rows_sum(self, ct: torch.Tensor, steps, gk: GaloisKeys, groups: int | None = None, src_index=None,
                        out: torch.Tensor | None = None) -> torch.Tensor:
        """out[g] = sum over t of rotate_rows(ct[source of item g * len(steps) + t], steps[t]): the bits of rotate_rows + add.  Item i
        reads source src_index[i % len(src_index)]; without src_index it reads ct[i] (groups * len(steps) ciphertexts).  groups defaults
        to the items / terms."""
        st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
        assert st.ndim == 1, st.shape
        groups, ip, n, out, _keep = self._rotation_sum_args(ct, st.size, groups, src_index, out)
        _check(_lib.load().hipbfv_batch_rotate_rows_sum(self._h, _ptr(ct), ct.shape[0], ip, n, st.ctypes.data_as(C.POINTER(C.c_int32)), gk.get_handle(),
                                                        _ptr(out), groups, st.size, _stream()))
        return out

    def apply_galois_sum(self, ct: torch.Tensor, galois_elts, gk: GaloisKeys, groups: int | None = None, src_index=None,
                         out: torch.Tensor | None = None) -> torch.Tensor:
        """rotate_rows_sum with term t given by its Galois element (odd, below 2 N; 1: the source itself)."""
        elts = np.ascontiguousarray(np.asarray(galois_elts, dtype=np.uint32))
        assert elts.ndim == 1, elts.shape
        groups, ip, n, out, _keep = self._rotation_sum_args(ct, elts.size, groups, src_index, out)
        _check(_lib.load().hipbfv_batch_apply_galois_sum(self._h, _ptr(ct), ct.shape[0], ip, n, elts.ctypes.data_as(C.POINTER(C.c_uint32)), gk.get_handle(),
                                                         _ptr(out), groups, elts.size, _stream()))
        return out

    # ---- weighted sums of rotations: the weight applied to every finished term just before it is added (include/hipbfv.h) ----
    @staticmethod
    def _rotation_weights(weights, terms: int):
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.int64))
        assert w.shape == (terms,), (w.shape, terms)
        assert w.size == 0 or (int(w.min()) >= -(1 << 31) and int(w.max()) < (1 << 31)), "a weight is an int32"
        return np.ascontiguousarray(w.astype(np.int32))

    def rotate_rows_sum_weighted(self, ct: torch.Tensor, steps, weights, gk: GaloisKeys, groups: int | None = None, src_index=None,
                                 out: torch.Tensor | None = None) -> torch.Tensor:
        """out[g] = sum over t of weights[t] (.) rotate_rows(ct[source of item g * len(steps) + t], steps[t]): every word of residue row i
        of the rotated term times (weights[t] mod q_i) -- the bits of |w| add calls, after negate when w < 0.  weights: len(steps) integers
        in the int32 range, shared by every group.  Sources, groups and src_index as rotate_rows_sum."""
        st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
        assert st.ndim == 1, st.shape
        wt = self._rotation_weights(weights, st.size)
        groups, ip, n, out, _keep = self._rotation_sum_args(ct, st.size, groups, src_index, out)
        _check(_lib.load().hipbfv_batch_rotate_rows_sum_weighted(self._h, _ptr(ct), ct.shape[0], ip, n, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                 wt.ctypes.data_as(C.POINTER(C.c_int32)), gk.get_handle(), _ptr(out), groups, st.size,
                                                                 _stream()))
        return out

    def apply_galois_sum_weighted(self, ct: torch.Tensor, galois_elts, weights, gk: GaloisKeys, groups: int | None = None, src_index=None,
                                  out: torch.Tensor | None = None) -> torch.Tensor:
        """rotate_rows_sum_weighted with term t given by its Galois element (odd, below 2 N; 1: the source itself)."""
        elts = np.ascontiguousarray(np.asarray(galois_elts, dtype=np.uint32))
        assert elts.ndim == 1, elts.shape
        wt = self._rotation_weights(weights, elts.size)
        groups, ip, n, out, _keep = self._rotation_sum_args(ct, elts.size, groups, src_index, out)
        _check(_lib.load().hipbfv_batch_apply_galois_sum_weighted(self._h, _ptr(ct), ct.shape[0], ip, n, elts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                  wt.ctypes.data_as(C.POINTER(C.c_int32)), gk.get_handle(), _ptr(out), groups, elts.size,
                                                                  _stream()))
        return out

    # ---- per-key batches (multi-tenant: the reference passes the keys per call, sunscreen_runtime/src/run.rs:100-105) ----
    @staticmethod
    def _key_sets(key_sets, key_index, count: int):
        # a None entry is a NULL handle: allowed for a set no item names (only the sets key_index names are read)
        handles = (C.c_void_p * len(key_sets))(*[k.get_handle() if k is not None else None for k in key_sets])
        idx = np.ascontiguousarray(np.asarray(key_index, dtype=np.uint32))
        assert idx.shape == (count,), (idx.shape, count)
        return handles, len(key_sets), idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx

    def relinearize_keys(self, ct3: torch.Tensor, key_sets: Sequence[RelinearizationKeys], key_index, out: torch.Tensor | None = None) -> torch.Tensor:
        """Item i is relinearised with key_sets[key_index[i]] (key_index: `count` host integers).  Only the sets key_index names
        are read: the others may be None or lack the key."""
        self._shape_ok(ct3, 3)
        out = out if out is not None else self._new(ct3.shape[0], 2, ct3)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, ct3.shape[0])
        _check(_lib.load().hipbfv_batch_relinearize_keys(self._h, _ptr(ct3), hs, n, ip, _ptr(out), ct3.shape[0], _stream()))
        return out

    def multiply_relin_keys(self, a: torch.Tensor, b: torch.Tensor, key_sets: Sequence[RelinearizationKeys], key_index,
                            out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(a, 2)
        self._shape_ok(b, 2)
        assert a.shape[0] == b.shape[0]
        out = out if out is not None else self._new(a.shape[0], 2, a)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, a.shape[0])
        _check(_lib.load().hipbfv_batch_multiply_relin_keys(self._h, _ptr(a), _ptr(b), hs, n, ip, _ptr(out), a.shape[0], _stream()))
        return out

    # ---- sums of products, one relinearization per group (include/hipbfv.h) ----
    def _sum_shape(self, a: torch.Tensor, b: torch.Tensor):
        for t in (a, b):
            assert t.dim() == 5 and t.shape[2] == 2 and t.shape[3] == self.K and t.shape[4] == self.n, tuple(t.shape)
        assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
        return a.shape[0], a.shape[1]

    def multiply_sum(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """a, b: [groups, terms, 2, K, N] (`b is a`: sums of squares).  out[g] = sum_t a[g, t] * b[g, t] as size-3 ciphertexts
        [groups, 3, K, N]: the words of multiply() on every term, added.  No in-place form."""
        groups, terms = self._sum_shape(a, b)
        out = out if out is not None else self._new(groups, 3, a)
        _check(_lib.load().hipbfv_batch_multiply_sum(self._h, _ptr(a), _ptr(b), _ptr(out), groups, terms, _stream()))
        return out

    def multiply_sum_relin(self, a: torch.Tensor, b: torch.Tensor, rk: RelinearizationKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        """relinearize(multiply_sum(a, b)), [groups, 2, K, N]: one key switch per group instead of one per term."""
        groups, terms = self._sum_shape(a, b)
        out = out if out is not None else self._new(groups, 2, a)
        _check(_lib.load().hipbfv_batch_multiply_sum_relin(self._h, _ptr(a), _ptr(b), rk.get_handle(), _ptr(out), groups, terms, _stream()))
        return out

    def multiply_sum_relin_keys(self, a: torch.Tensor, b: torch.Tensor, key_sets: Sequence[RelinearizationKeys | None], key_index,
                                out: torch.Tensor | None = None) -> torch.Tensor:
        """Group g is relinearised with key_sets[key_index[g]] (key_index: `groups` host integers); only named sets are read."""
        groups, terms = self._sum_shape(a, b)
        out = out if out is not None else self._new(groups, 2, a)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, groups)
        _check(_lib.load().hipbfv_batch_multiply_sum_relin_keys(self._h, _ptr(a), _ptr(b), hs, n, ip, _ptr(out), groups, terms, _stream()))
        return out

    # ---- weighted sums of products: sum_t weights[t] * a[g, t] * b[g, t] (include/hipbfv.h) ----
    @staticmethod
    def _weights(weights, terms: int):
        w = [int(x) for x in weights]
        assert len(w) == terms, (len(w), terms)
        assert all(-(1 << 31) <= x < (1 << 31) for x in w), "a weight is a 32-bit signed integer"
        return (C.c_int32 * terms)(*w)

    def multiply_sum_weighted(self, a: torch.Tensor, b: torch.Tensor, weights, out: torch.Tensor | None = None) -> torch.Tensor:
        """out[g] = sum_t weights[t] * a[g, t] * b[g, t] as size-3 ciphertexts: every row i of term t's product times (weights[t] mod q_i)
        before it is added.  weights: `terms` host integers (32-bit signed), shared by every group; a weight multiplies its term's noise by |w|."""
        groups, terms = self._sum_shape(a, b)
        out = out if out is not None else self._new(groups, 3, a)
        _check(_lib.load().hipbfv_batch_multiply_sum_weighted(self._h, _ptr(a), _ptr(b), self._weights(weights, terms), _ptr(out), groups, terms, _stream()))
        return out

    def multiply_sum_weighted_relin(self, a: torch.Tensor, b: torch.Tensor, weights, rk: RelinearizationKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        """relinearize(multiply_sum_weighted(a, b, weights)), [groups, 2, K, N]: one key switch per group."""
        groups, terms = self._sum_shape(a, b)
        out = out if out is not None else self._new(groups, 2, a)
        _check(_lib.load().hipbfv_batch_multiply_sum_weighted_relin(self._h, _ptr(a), _ptr(b), self._weights(weights, terms), rk.get_handle(), _ptr(out),
                                                                    groups, terms, _stream()))
        return out

    def multiply_sum_weighted_relin_keys(self, a: torch.Tensor, b: torch.Tensor, weights, key_sets: Sequence[RelinearizationKeys | None], key_index,
                                         out: torch.Tensor | None = None) -> torch.Tensor:
        """Group g is relinearised with key_sets[key_index[g]]; the weights are shared by every group."""
        groups, terms = self._sum_shape(a, b)
        out = out if out is not None else self._new(groups, 2, a)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, groups)
        _check(_lib.load().hipbfv_batch_multiply_sum_weighted_relin_keys(self._h, _ptr(a), _ptr(b), self._weights(weights, terms), hs, n, ip, _ptr(out),
                                                                         groups, terms, _stream()))
        return out

    # ---- prepared multiplicands: a shared second operand transformed once (include/hipbfv.h) ----
    def prepare(self, ct: torch.Tensor) -> "Multiplicand":
        """ct: [count, 2, K, N].  The ciphertexts are copied and, where the parameter set has a split multiply, extended and
        transformed once; asynchronous on the current stream.  The object may be used on any stream (it carries an event)."""
        self._shape_ok(ct, 2)
        h = C.c_void_p()
        _check(_lib.load().hipbfv_Multiplicand_Create(self._h, _ptr(ct), ct.shape[0], _stream(), C.byref(h)))
        return Multiplicand(h, self.ctx)

    @staticmethod
    def _b_index(b_index):
        idx = np.ascontiguousarray(np.asarray(b_index, dtype=np.uint32)).reshape(-1)
        return idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size, idx

    def multiply_shared(self, a: torch.Tensor, m: "Multiplicand", b_index, out: torch.Tensor | None = None) -> torch.Tensor:
        """out[i] = a[i] * m[b_index[i % len(b_index)]] as size-3 ciphertexts: the words of multiply() on the replicated operand."""
        self._shape_ok(a, 2)
        out = out if out is not None else self._new(a.shape[0], 3, a)
        ip, n, _keep = self._b_index(b_index)
        _check(_lib.load().hipbfv_batch_multiply_shared(self._h, _ptr(a), m.get_handle(), ip, n, _ptr(out), a.shape[0], _stream()))
        return out

    def multiply_relin_shared(self, a: torch.Tensor, m: "Multiplicand", b_index, rk: RelinearizationKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        """multiply_relin() with the second operands taken from m; `out=a` is allowed."""
        self._shape_ok(a, 2)
        out = out if out is not None else self._new(a.shape[0], 2, a)
        ip, n, _keep = self._b_index(b_index)
        _check(_lib.load().hipbfv_batch_multiply_relin_shared(self._h, _ptr(a), m.get_handle(), ip, n, rk.get_handle(), _ptr(out), a.shape[0], _stream()))
        return out

    def multiply_sum_shared(self, a: torch.Tensor, m: "Multiplicand", b_index, out: torch.Tensor | None = None) -> torch.Tensor:
        """a: [groups, terms, 2, K, N]; out[g] = sum_t a[g, t] * m[b_index[(g * terms + t) % len(b_index)]], [groups, 3, K, N].
        b_index = range(terms): a ciphertext matrix times the prepared vector."""
        groups, terms = self._sum_shape(a, a)
        out = out if out is not None else self._new(groups, 3, a)
        ip, n, _keep = self._b_index(b_index)
        _check(_lib.load().hipbfv_batch_multiply_sum_shared(self._h, _ptr(a), m.get_handle(), ip, n, _ptr(out), groups, terms, _stream()))
        return out

    def multiply_sum_relin_shared(self, a: torch.Tensor, m: "Multiplicand", b_index, rk: RelinearizationKeys, out: torch.Tensor | None = None) -> torch.Tensor:
        """relinearize(multiply_sum_shared(a, m, b_index)), [groups, 2, K, N]: one key switch per group."""
        groups, terms = self._sum_shape(a, a)
        out = out if out is not None else self._new(groups, 2, a)
        ip, n, _keep = self._b_index(b_index)
        _check(_lib.load().hipbfv_batch_multiply_sum_relin_shared(self._h, _ptr(a), m.get_handle(), ip, n, rk.get_handle(), _ptr(out), groups, terms,
                                                                  _stream()))
        return out

    # ---- products of two prepared operands: no head, one middle kernel over both operands' rows (include/hipbfv.h) ----
    @classmethod
    def _pair_index(cls, a_index, b_index):
        ap, na, ka = cls._b_index(a_index)
        bp, nb, kb = cls._b_index(b_index)
        if na != nb:
            raise ValueError(f"a_index has {na} entries, b_index {nb}")
        return ap, bp, na, (ka, kb)

    def _new_prepared(self, count: int, size: int) -> torch.Tensor:
        # (the operands live inside the objects: the output goes to the current device)
        return torch.empty((count, size, self.K, self.n), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))

    def multiply_prepared(self, ma: "Multiplicand", a_index, mb: "Multiplicand", b_index, count: int | None = None,
                          out: torch.Tensor | None = None) -> torch.Tensor:
        """out[i] = ma[a_index[i % L]] * mb[b_index[i % L]] as size-3 ciphertexts, L = len(a_index) = len(b_index); count defaults to L.
        The words of multiply() on the two gathered arrays."""
        ap, bp, n, _keep = self._pair_index(a_index, b_index)
        count = n if count is None else count
        out = out if out is not None else self._new_prepared(count, 3)
        _check(_lib.load().hipbfv_batch_multiply_prepared(self._h, ma.get_handle(), ap, mb.get_handle(), bp, n, _ptr(out), count, _stream()))
        return out

    def multiply_relin_prepared(self, ma: "Multiplicand", a_index, mb: "Multiplicand", b_index, rk: RelinearizationKeys, count: int | None = None,
                                out: torch.Tensor | None = None) -> torch.Tensor:
        """multiply_relin() with both operands taken from prepared objects, [count, 2, K, N]."""
        ap, bp, n, _keep = self._pair_index(a_index, b_index)
        count = n if count is None else count
        out = out if out is not None else self._new_prepared(count, 2)
        _check(_lib.load().hipbfv_batch_multiply_relin_prepared(self._h, ma.get_handle(), ap, mb.get_handle(), bp, n, rk.get_handle(), _ptr(out), count,
                                                                _stream()))
        return out

    def multiply_sum_prepared(self, ma: "Multiplicand", a_index, mb: "Multiplicand", b_index, groups: int, terms: int,
                              out: torch.Tensor | None = None) -> torch.Tensor:
        """out[g] = sum_t ma[a_index[(g * terms + t) % L]] * mb[b_index[(g * terms + t) % L]], [groups, 3, K, N]."""
        ap, bp, n, _keep = self._pair_index(a_index, b_index)
        out = out if out is not None else self._new_prepared(groups, 3)
        _check(_lib.load().hipbfv_batch_multiply_sum_prepared(self._h, ma.get_handle(), ap, mb.get_handle(), bp, n, _ptr(out), groups, terms, _stream()))
        return out

    def multiply_sum_relin_prepared(self, ma: "Multiplicand", a_index, mb: "Multiplicand", b_index, rk: RelinearizationKeys, groups: int, terms: int,
                                    out: torch.Tensor | None = None) -> torch.Tensor:
        """relinearize(multiply_sum_prepared(...)), [groups, 2, K, N]: one key switch per group."""
        ap, bp, n, _keep = self._pair_index(a_index, b_index)
        out = out if out is not None else self._new_prepared(groups, 2)
        _check(_lib.load().hipbfv_batch_multiply_sum_relin_prepared(self._h, ma.get_handle(), ap, mb.get_handle(), bp, n, rk.get_handle(), _ptr(out),
                                                                    groups, terms, _stream()))
        return out

    def apply_galois_keys(self, ct: torch.Tensor, galois_elt: int, key_sets: Sequence[GaloisKeys], key_index, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, ct.shape[0])
        _check(_lib.load().hipbfv_batch_apply_galois_keys(self._h, _ptr(ct), galois_elt, hs, n, ip, _ptr(out), ct.shape[0], _stream()))
        return out

    def rotate_rows_keys(self, ct: torch.Tensor, steps: int, key_sets: Sequence[GaloisKeys], key_index, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, ct.shape[0])
        _check(_lib.load().hipbfv_batch_rotate_rows_keys(self._h, _ptr(ct), steps, hs, n, ip, _ptr(out), ct.shape[0], _stream()))
        return out

    def rotate_columns_keys(self, ct: torch.Tensor, key_sets: Sequence[GaloisKeys], key_index, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, ct.shape[0])
        _check(_lib.load().hipbfv_batch_rotate_columns_keys(self._h, _ptr(ct), hs, n, ip, _ptr(out), ct.shape[0], _stream()))
        return out

    # ---- mixed-step rotation batches with one key set per client (include/hipbfv.h) ----
    def apply_galois_items_keys(self, ct: torch.Tensor, galois_elts, key_sets: Sequence[GaloisKeys | None], key_index,
                                out: torch.Tensor | None = None) -> torch.Tensor:
        """Item i by galois_elts[i] through key_sets[key_index[i]].  An item of element 1 is copied and references no set."""
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        elts = np.ascontiguousarray(np.asarray(galois_elts, dtype=np.uint32))
        assert elts.shape == (ct.shape[0],), (elts.shape, ct.shape[0])
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, ct.shape[0])
        _check(_lib.load().hipbfv_batch_apply_galois_items_keys(self._h, _ptr(ct), elts.ctypes.data_as(C.POINTER(C.c_uint32)), hs, n, ip, _ptr(out),
                                                                ct.shape[0], _stream()))
        return out

    def rotate_rows_items_keys(self, ct: torch.Tensor, steps, key_sets: Sequence[GaloisKeys | None], key_index,
                               out: torch.Tensor | None = None) -> torch.Tensor:
        """Item i rotated by steps[i] with key_sets[key_index[i]]: the bits of rotate_rows(ct[i:i+1], steps[i], that set).  Every
        (set, step) pair decides on its own between a copy, the direct key and the NAF chain; all direct items share one launch
        sequence, all chain items share their rounds."""
        self._shape_ok(ct, 2)
        out = out if out is not None else self._new(ct.shape[0], 2, ct)
        st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
        assert st.shape == (ct.shape[0],), (st.shape, ct.shape[0])
        hs, n, ip, _keep = self._key_sets(key_sets, key_index, ct.shape[0])
        _check(_lib.load().hipbfv_batch_rotate_rows_items_keys(self._h, _ptr(ct), st.ctypes.data_as(C.POINTER(C.c_int32)), hs, n, ip, _ptr(out),
                                                               ct.shape[0], _stream()))
        return out

    # ---- a5 ----
    def add(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(a)
        assert a.shape == b.shape
        out = out if out is not None else torch.empty_like(a)
        _check(_lib.load().hipbfv_batch_add(self._h, _ptr(a), _ptr(b), _ptr(out), a.shape[1], a.shape[0], _stream()))
        return out

    def sub(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(a)
        assert a.shape == b.shape
        out = out if out is not None else torch.empty_like(a)
        _check(_lib.load().hipbfv_batch_sub(self._h, _ptr(a), _ptr(b), _ptr(out), a.shape[1], a.shape[0], _stream()))
        return out

    def negate(self, a: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        self._shape_ok(a)
        out = out if out is not None else torch.empty_like(a)
        _check(_lib.load().hipbfv_batch_negate(self._h, _ptr(a), _ptr(out), a.shape[1], a.shape[0], _stream()))
        return out

    def _plain(self, fn, ct: torch.Tensor, plain: torch.Tensor, out):
        self._shape_ok(ct)
        assert plain.shape[-1] == self.n
        stride = 0 if plain.dim() == 1 or plain.shape[0] == 1 else self.n
        if stride:
            assert plain.shape[0] == ct.shape[0]
        out = out if out is not None else torch.empty_like(ct)
        _check(fn(self._h, _ptr(ct), ct.shape[1], _ptr(plain), stride, _ptr(out), ct.shape[0], _stream()))
        return out

    def add_plain(self, ct, plain, out=None):
        return self._plain(_lib.load().hipbfv_batch_add_plain, ct, plain, out)

    def sub_plain(self, ct, plain, out=None):
        return self._plain(_lib.load().hipbfv_batch_sub_plain, ct, plain, out)

    # ---- a4 ----
    def multiply_plain(self, ct, plain, out=None):
        return self._plain(_lib.load().hipbfv_batch_multiply_plain, ct, plain, out)

    # ---- 8f row 3: the steps either side of the path, on device-resident batches ----
    def encode(self, values: torch.Tensor, signed: bool = False) -> torch.Tensor:
        """BatchEncoder: int64[batch, N] slot values -> int64[batch, N] plaintext coefficients."""
        assert values.dim() == 2 and values.shape[1] == self.n
        out = torch.empty_like(values)
        _check(_lib.load().hipbfv_batch_encode(self._h, _ptr(values), _ptr(out), values.shape[0], int(signed), _stream()))
        return out

    def decode(self, plain: torch.Tensor, signed: bool = False) -> torch.Tensor:
        assert plain.dim() == 2 and plain.shape[1] == self.n
        out = torch.empty_like(plain)
        _check(_lib.load().hipbfv_batch_decode(self._h, _ptr(plain), _ptr(out), plain.shape[0], int(signed), _stream()))
        return out

    def decrypt(self, ct: torch.Tensor, secret_key) -> torch.Tensor:
        """int64[batch, size, K, N] -> int64[batch, N] plaintext coefficients (zero padded); secret_key: seal.SecretKey."""
        assert ct.dim() == 4 and ct.shape[2] == self.K and ct.shape[3] == self.n
        out = torch.empty((ct.shape[0], self.n), dtype=torch.int64, device=ct.device)
        _check(_lib.load().hipbfv_batch_decrypt(self._h, _ptr(ct), ct.shape[1], secret_key.get_handle(), _ptr(out), ct.shape[0], _stream()))
        return out

    def noise_budget(self, ct: torch.Tensor, secret_key, with_noise: bool = False):
        """Decryptor_InvariantNoiseBudget per item: int32[batch] (and, with_noise, Decryptor_InvariantNoise as float64[batch]).
        Asynchronous like the other calls; a budget of 0 means the item no longer decrypts correctly."""
        assert ct.dim() == 4 and ct.shape[2] == self.K and ct.shape[3] == self.n
        budget = torch.empty((ct.shape[0],), dtype=torch.int32, device=ct.device)
        noise = torch.empty((ct.shape[0],), dtype=torch.float64, device=ct.device) if with_noise else None
        _check(_lib.load().hipbfv_batch_noise_budget(self._h, _ptr(ct), ct.shape[1], secret_key.get_handle(), C.c_void_p(budget.data_ptr()),
                                                     C.c_void_p(noise.data_ptr()) if with_noise else None, ct.shape[0], _stream()))
        return (budget, noise) if with_noise else budget

    def decrypt_checked(self, ct: torch.Tensor, secret_key):
        """decrypt() and noise_budget() from one phase computation: (int64[batch, N] plaintexts, int32[batch] budgets).  An item
        with budget 0 decrypted to garbage: the reference's Runtime::decrypt returns Error::TooMuchNoise for it."""
        assert ct.dim() == 4 and ct.shape[2] == self.K and ct.shape[3] == self.n
        plain = torch.empty((ct.shape[0], self.n), dtype=torch.int64, device=ct.device)
        budget = torch.empty((ct.shape[0],), dtype=torch.int32, device=ct.device)
        _check(_lib.load().hipbfv_batch_decrypt_checked(self._h, _ptr(ct), ct.shape[1], secret_key.get_handle(), _ptr(plain),
                                                        C.c_void_p(budget.data_ptr()), ct.shape[0], _stream()))
        return plain, budget

    def encrypt(self, plain: torch.Tensor, public_key, seed: int | bytes | None = None, first_op: int = 0) -> torch.Tensor:
        """int64[batch, N] (or one shared int64[N]) plaintexts -> fresh encryptions int64[batch', 2, K, N].
        seed: None = 512 fresh bits from the OS (production); 64 bytes = SEAL's prng_seed_type; an int = the TEST-ONLY
        64-bit seed (reproducible batches)."""
        shared = plain.dim() == 1
        count = 1 if shared else plain.shape[0]
        out = torch.empty((count, 2, self.K, self.n), dtype=torch.int64, device=plain.device)
        if isinstance(seed, int):
            _check(_lib.load().hipbfv_batch_encrypt(self._h, _ptr(plain), 0 if shared else self.n, public_key.get_handle(), seed, first_op,
                                                    _ptr(out), count, _stream()))
        else:
            assert seed is None or len(seed) == 64
            _check(_lib.load().hipbfv_batch_encrypt_seeded(self._h, _ptr(plain), 0 if shared else self.n, public_key.get_handle(), seed, first_op,
                                                           _ptr(out), count, _stream()))
        return out

    def mod_switch(self, ct: torch.Tensor) -> torch.Tensor:
        """mod_switch_to_next on a batch: int64[batch, size, K, N] -> int64[batch, size, K-1, N], the layout of
        `self.ctx.next_level()` (build a BatchEvaluator on that context to continue there)."""
        assert ct.dim() == 4 and ct.shape[2] == self.K and ct.shape[3] == self.n
        out = torch.empty((ct.shape[0], ct.shape[1], self.K - 1, self.n), dtype=torch.int64, device=ct.device)
        _check(_lib.load().hipbfv_batch_mod_switch(self._h, _ptr(ct), ct.shape[1], _ptr(out), ct.shape[0], _stream()))
        return out

    # ---- plaintext-matrix x ciphertext-vector products (examples/pir) ----
    def plain_to_ntt(self, plain: torch.Tensor) -> torch.Tensor:
        """int64[..., N] plaintexts -> int64[..., K, N]: the transform-domain operand multiply_plain builds internally."""
        assert plain.shape[-1] == self.n
        flat = plain.reshape(-1, self.n).contiguous()
        out = torch.empty((flat.shape[0], self.K, self.n), dtype=torch.int64, device=plain.device)
        _check(_lib.load().hipbfv_batch_plain_to_ntt(self._h, _ptr(flat), self.n, _ptr(out), flat.shape[0], _stream()))
        # an all-zero plaintext has no transformed form (SEAL refuses every product with it, and the consumers of `out` cannot
        # see it any more): the producer recorded it, and this is where the caller learns -- static data is transformed once.
        # check() synchronises the stream and reads-and-resets the evaluator's ONE status word: what it raises covers every
        # batched operation since the previous check, not this call alone ("Asynchronous status").
        self.check()
        return out.reshape(tuple(plain.shape[:-1]) + (self.K, self.n))

    def ct_to_ntt(self, ct: torch.Tensor) -> torch.Tensor:
        assert ct.dim() == 4 and ct.shape[2] == self.K and ct.shape[3] == self.n
        out = torch.empty_like(ct)
        _check(_lib.load().hipbfv_batch_ct_to_ntt(self._h, _ptr(ct), ct.shape[1], _ptr(out), ct.shape[0], _stream()))
        return out

    def dot_plain_ntt(self, ctn: torch.Tensor, pntt: torch.Tensor) -> torch.Tensor:
        """ctn: int64[cols, 2, K, N] (ct_to_ntt), pntt: int64[rows, cols, K, N] (plain_to_ntt) ->
        int64[rows, 2, K, N] = sum_j multiply_plain(ct_j, plain[row][j]), coefficient form."""
        cols, rows = ctn.shape[0], pntt.shape[0]
        assert ctn.shape[1] == 2 and pntt.shape[1] == cols and pntt.shape[2] == self.K
        out = torch.empty((rows, 2, self.K, self.n), dtype=torch.int64, device=ctn.device)
        _check(_lib.load().hipbfv_batch_dot_plain_ntt(self._h, _ptr(ctn), cols, _ptr(pntt), rows, _ptr(out), _stream()))
        return out

    def dot_plain_ntt_queries(self, ctn: torch.Tensor, pntt: torch.Tensor) -> torch.Tensor:
        """Q queries against ONE pass over the database.  ctn: int64[Q, cols, 2, K, N] (ct_to_ntt of each query), pntt:
        int64[rows, cols, K, N] (plain_to_ntt) -> int64[Q, rows, 2, K, N]; out[q] has the bits of dot_plain_ntt(ctn[q], pntt).  The
        result is laid out as multiply_sum_relin_keys takes a[groups = Q, terms = rows]."""
        assert ctn.dim() == 5 and pntt.dim() == 4, (ctn.shape, pntt.shape)
        queries, cols, rows = ctn.shape[0], ctn.shape[1], pntt.shape[0]
        assert tuple(ctn.shape[2:]) == (2, self.K, self.n) and tuple(pntt.shape[1:]) == (cols, self.K, self.n), (ctn.shape, pntt.shape)
        assert ctn.is_contiguous() and pntt.is_contiguous()
        out = torch.empty((queries, rows, 2, self.K, self.n), dtype=torch.int64, device=ctn.device)
        _check(_lib.load().hipbfv_batch_dot_plain_ntt_queries(self._h, _ptr(ctn), queries, cols, _ptr(pntt), rows, _ptr(out), _stream()))
        return out

    # ---- a6: NTT entry points (BASELINE config 2) ----
    def ntt(self, data: torch.Tensor, nprimes: int, inverse: bool = False) -> torch.Tensor:
        """In-place negacyclic NTT of int64[polys, N]; polynomial p uses key-level prime p % nprimes."""
        assert data.dim() == 2 and data.shape[1] == self.n
        _check(_lib.load().hipbfv_batch_ntt(self._h, _ptr(data), data.shape[0], nprimes, inverse, _stream()))
        return data


class Multiplicand:
    """A prepared second operand (BatchEvaluator.prepare): `count` ciphertexts kept on the device, transformed once."""

    def __init__(self, handle, ctx: Context):
        self._h = handle
        self.ctx = ctx  # (keeps the context alive)

    def get_handle(self):
        return self._h

    @property
    def count(self) -> int:
        n = C.c_uint64()
        _check(_lib.load().hipbfv_Multiplicand_Count(self._h, C.byref(n)))
        return n.value

    @property
    def nbytes(self) -> int:
        """Device memory the object holds: the copy of the ciphertexts and their transformed rows."""
        n = C.c_uint64()
        _check(_lib.load().hipbfv_Multiplicand_Bytes(self._h, C.byref(n)))
        return n.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.load().hipbfv_Multiplicand_Destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rotate_items_plan(n: int, steps, present_elts) -> tuple[list[int], list[int], int]:
    """The library's plan for rotate_rows_items (host only): per item its kind (0 copied, 1 in the mixed launch, 2 in a NAF chain
    group) and its group (kind 1: the Galois element, kind 2: the chain group), and the number of chain groups -- at degree n,
    over a key set that holds exactly the keys of present_elts."""
    st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
    pe = np.ascontiguousarray(np.asarray(present_elts, dtype=np.uint32))
    kind = (C.c_int32 * max(1, st.size))()
    group = (C.c_uint32 * max(1, st.size))()
    ng = C.c_uint64()
    _check(_lib.load().hipbfv_debug_rotate_items_plan(n, st.ctypes.data_as(C.POINTER(C.c_int32)), st.size, pe.ctypes.data_as(C.POINTER(C.c_uint32)), pe.size,
                                                      kind, group, C.byref(ng)))
    return list(kind[: st.size]), list(group[: st.size]), ng.value


def rotate_items_keys_plan(n: int, steps, key_index, present_sets) -> tuple[list[int], list[int], list[int], int, int]:
    """The library's plan for rotate_rows_items_keys (host only) at degree n, where key set k holds exactly the keys of the Galois
    elements present_sets[k]: per item its kind (0 copied, 1 in the mixed launch, 2 in a NAF chain), its entry of the mixed
    launch's key table (kind 1; entries are numbered by (element, set)) and its chain's rounds (kind 2); then the number of
    table entries and the rounds the call runs (the longest chain's)."""
    st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
    ki = np.ascontiguousarray(np.asarray(key_index, dtype=np.uint32))
    assert st.shape == ki.shape and st.ndim == 1, (st.shape, ki.shape)
    offsets = np.zeros(len(present_sets) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in present_sets])
    pe = np.ascontiguousarray(np.asarray([e for p in present_sets for e in p], dtype=np.uint32))
    kind = (C.c_int32 * max(1, st.size))()
    entry = (C.c_uint32 * max(1, st.size))()
    rounds_of = (C.c_uint32 * max(1, st.size))()
    entries, rounds = C.c_uint64(), C.c_uint64()
    _check(_lib.load().hipbfv_debug_rotate_items_keys_plan(n, st.ctypes.data_as(C.POINTER(C.c_int32)), ki.ctypes.data_as(C.POINTER(C.c_uint32)), st.size,
                                                           len(present_sets), pe.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                           offsets.ctypes.data_as(C.POINTER(C.c_uint64)), kind, entry, rounds_of, C.byref(entries),
                                                           C.byref(rounds)))
    return list(kind[: st.size]), list(entry[: st.size]), list(rounds_of[: st.size]), entries.value, rounds.value


def rotate_sum_plan(n: int, steps, present_elts, groups: int, chunk: int):
    """The library's plan for rotate_rows_sum (host only) at degree n over a key set that holds exactly the keys of present_elts: per
    term its kind (0 the source itself, 1 through its own key inside the summing sequence, 2 a NAF chain beforehand), its Galois
    element and its chain's rounds; then the launch sequences as multiply_sum_plan reports them."""
    st = np.ascontiguousarray(np.asarray(steps, dtype=np.int32))
    pe = np.ascontiguousarray(np.asarray(present_elts, dtype=np.uint32))
    kind = (C.c_int32 * max(1, st.size))()
    elt = (C.c_uint32 * max(1, st.size))()
    rounds = (C.c_uint32 * max(1, st.size))()
    L = _lib.load()
    args = (n, st.ctypes.data_as(C.POINTER(C.c_int32)), st.size, pe.ctypes.data_as(C.POINTER(C.c_uint32)), pe.size, groups, chunk, kind, elt, rounds)
    cnt = C.c_uint64()
    L.hipbfv_debug_rotate_sum_plan(*args, None, 0, C.byref(cnt))  # (the count; the call below raises what this one refused)
    buf = (C.c_uint64 * (5 * max(1, cnt.value)))()
    _check(L.hipbfv_debug_rotate_sum_plan(*args, buf, cnt.value, C.byref(cnt)))
    seq = [(buf[5 * i], buf[5 * i + 1], buf[5 * i + 2], buf[5 * i + 3], bool(buf[5 * i + 4])) for i in range(cnt.value)]
    return list(kind[: st.size]), list(elt[: st.size]), list(rounds[: st.size]), seq


def multiply_sum_plan(groups: int, terms: int, chunk: int) -> list[tuple[int, int, int, int, bool]]:
    """The library's launch sequences for multiply_sum / multiply_sum_relin (host only) under a chunk of `chunk` items: per sequence
    (first group, groups, first term, terms, accumulate).  A chunk is a whole number of groups; a group with more terms than a chunk
    holds runs alone in slices of `chunk` terms, every slice but the first adding onto the group's sums."""
    L = _lib.load()
    n = C.c_uint64()
    L.hipbfv_debug_multiply_sum_plan(groups, terms, chunk, None, 0, C.byref(n))  # (the count; refused only for a plan that is not empty)
    buf = (C.c_uint64 * (5 * max(1, n.value)))()
    _check(L.hipbfv_debug_multiply_sum_plan(groups, terms, chunk, buf, n.value, C.byref(n)))
    return [(buf[5 * i], buf[5 * i + 1], buf[5 * i + 2], buf[5 * i + 3], bool(buf[5 * i + 4])) for i in range(n.value)]


def dot_queries_plan(queries: int, rows: int, K: int) -> list[tuple[int, int, int, int, int, int]]:
    """The library's product launches for dot_plain_ntt_queries (host only): per launch (first query, queries, first row, rows, QT,
    RT) -- those queries against those rows, QT queries and RT rows per thread.  QT == 1 is the single-query kernel of dot_plain_ntt.
    One query is one such launch; otherwise all queries go into one launch of the query-tiled kernel (split only where row blocks x
    query tiles would exceed 2^31 - 1 workgroups)."""
    L = _lib.load()
    n = C.c_uint64()
    L.hipbfv_debug_dot_queries_plan(queries, rows, K, None, 0, C.byref(n))  # (the count; the call below raises what this one refused)
    buf = (C.c_uint64 * (6 * max(1, n.value)))()
    _check(L.hipbfv_debug_dot_queries_plan(queries, rows, K, buf, n.value, C.byref(n)))
    return [tuple(int(buf[6 * i + k]) for k in range(6)) for i in range(n.value)]


def weight_residues(primes, weights) -> list[list[tuple[int, int]]]:
    """The weight table of the weighted sums (host only): [term][prime] = (w mod q canonical, floor(that * 2^64 / q))."""
    L = _lib.load()
    p = (C.c_uint64 * len(primes))(*[int(q) for q in primes])
    w = (C.c_int32 * len(weights))(*[int(x) for x in weights])
    out = (C.c_uint64 * (2 * len(primes) * len(weights)))()
    _check(L.hipbfv_debug_weight_residues(p, len(primes), w, len(weights), out))
    return [[(out[2 * (t * len(primes) + i)], out[2 * (t * len(primes) + i) + 1]) for i in range(len(primes))] for t in range(len(weights))]
