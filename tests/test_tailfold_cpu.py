"""Host proof of the folded FP64 tail (sunscreen_amd/csrc/moddown_d.hpp tail_fold4_d) and of the floor's single constant product.

The tails of the split pipelines ran two inverse stages (four twiddle products) and then multiplied their four values by a fixed
per-modulus scaling: eight constant products.  With the scaling folded into the constants of every difference whose inputs are
still unscaled there are five, and the BEHZ floor multiplies by q^-1 (B/B_j)^-1 once instead of by each in turn.  Every value is
congruent to the one it replaces; what has to be shown is that the FP64 arithmetic stays exact and inside the bounds its consumers
state.  tests/native/tailfold_check.cpp includes the header the kernels include and compares with 128-bit integers: primes of
36 ... 50 bits (top, bottom and inside of each size class) and the four data primes, the special prime and the library's own five
auxiliary primes of the n = 8192 default context, with every scale kind; random operands, operands at the tail-entry bound of the
range plan (+-bound in the patterns that maximise each sum and difference) and operands that put each product on 0, +-1 and
(q +- 1)/2 mod q; canonical results equal, |out1| <= 2q, every product within its stated bound."""
import ctypes as C
import os
import subprocess

from sunscreen_amd import _lib, seal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _context_8192(monkeypatch):
    """(key primes, B, m_sk, t) of the n = 8192 default context with the library's own auxiliary base (Context::create, host only)."""
    for k in ("HIPBFV_SEAL_AUX", "HIPBFV_NO_F64"):
        monkeypatch.delenv(k, raising=False)
    n = 8192
    key = [int(m.value()) for m in seal.CoefficientModulus.bfv_default(n)]
    t = int(seal.PlainModulus.batching(n, 17).value())
    arr = (C.c_uint64 * len(key))(*key)
    out = (C.c_uint64 * 32)()
    cnt, flags = C.c_uint64(), C.c_int()
    assert _lib.load().hipbfv_debug_aux_base(n, arr, len(key), t, C.byref(cnt), out, 32, C.byref(flags)) == 0
    aux = [int(v) for v in out[: cnt.value]]
    assert flags.value & 1, "the default context takes the library's own FP64 auxiliary base"
    return key, aux[:-1], aux[-1], t


def test_folded_tail_and_single_floor_product_are_exact(tmp_path, monkeypatch):
    key, B, m_sk, t = _context_8192(monkeypatch)
    assert len(key) == 5 and len(B) == 4 and all(p < (1 << 50) for p in key + B + [m_sk])
    ull = lambda xs: ",".join(f"{x}ull" for x in xs)  # noqa: E731
    exe = str(tmp_path / "tailfold_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           f"-DTAILFOLD_T={t}ull", f"-DTAILFOLD_KEY={ull(key)}", f"-DTAILFOLD_B={ull(B)}", f"-DTAILFOLD_MSK={m_sk}ull",
                           "-I", os.path.join(ROOT, "sunscreen_amd", "csrc"), os.path.join(ROOT, "tests", "native", "tailfold_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("ok ") and int(last.split()[1]) >= 1_500_000, out.stdout
