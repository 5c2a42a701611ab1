"""The batched noise measure's C ABI without a GPU: null pointers are refused before anything else, and the header, the ctypes
symbol table and the library agree on hipbfv_batch_noise_budget / hipbfv_batch_decrypt_checked."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_POINTER = 0x80004003
ENTRY = ("hipbfv_batch_noise_budget", "hipbfv_batch_decrypt_checked")


def test_null_pointers_are_refused():
    from sunscreen_amd import _lib

    L = _lib.load()
    d = C.c_void_p(0x1000)  # a device address: never dereferenced on the host, and every call below fails its pointer checks first
    # a null evaluator or secret key handle, a null ct / budget / plain
    for ev, ct, sk, out in ((None, d, None, d), (None, None, None, d), (None, d, None, None)):
        assert L.hipbfv_batch_noise_budget(ev, ct, 2, sk, out, None, 1, None) & 0xFFFFFFFF == E_POINTER
        assert L.hipbfv_batch_decrypt_checked(ev, ct, 2, sk, out, d, 1, None) & 0xFFFFFFFF == E_POINTER
        assert L.hipbfv_batch_decrypt_checked(ev, ct, 2, sk, d, out, 1, None) & 0xFFFFFFFF == E_POINTER


def test_header_declarations_match_the_symbol_table():
    from sunscreen_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipbfv.h")).read(), flags=re.S)
    for name in ENTRY:
        m = re.search(rf"^long\s+{name}\s*\((.*?)\);", header, flags=re.M | re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(_lib._SIGNATURES[name]) == 8, (name, args)
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
    # the two calls differ in their outputs only: ct, size, secret key, ..., count, stream
    nb = re.search(r"long\s+hipbfv_batch_noise_budget\s*\((.*?)\);", header, flags=re.S).group(1)
    dc = re.search(r"long\s+hipbfv_batch_decrypt_checked\s*\((.*?)\);", header, flags=re.S).group(1)
    assert "int32_t *budget" in nb and "double *noise" in nb
    assert "uint64_t *plain" in dc and "int32_t *budget" in dc
