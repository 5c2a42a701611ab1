"""The multiply head, the BEHZ floor, the multiply's outputs and decrypt's gamma correction on operands crafted so that the values
INSIDE the kernels land on their edges (tests/landing.py sections F, G and H; tests/test_landing_cpu.py shows that every builder
lands all of its words, from the primes alone).

F  r_mtilde in {0, 1, 2^31 - 1, 2^31, 2^31 + 1, 2^32 - 1} in front of every head thread, the scaled rows y_i on 0, q_i - 1, 1 and
   the integers around q_i / 2, and every y_i at q_i - 1 at once: behz_extend_coeff, _coeff_d, _coeff_mixed, _multi_d with and
   without the grid sums, _multi_mixed.
G  multiplications by (1, 1): the caller's a0 and a1 ARE the tensor's d0 and d2, so the floor reads y_i on the same edges and all
   rows at q_i - 1 at once; and operands harvested from the oracle whose product is 0, q_i - 1 or 1 in EVERY row.
H  ciphertexts whose gamma residue in decrypt's rounding is 0, 1, floor(gamma / 2) - 1, floor(gamma / 2), floor(gamma / 2) + 1,
   gamma - 1.

Every assertion on values is word-for-word equality with the CPU oracle over all words of all items and holds under every switch
the suite runs with; the profiler is read to see that the kernel a test is about ran (the names depend on the default arms)."""
import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing
from tests.oracle_program import run_program
from tests.test_gpu_landing import DEFAULT_ARMS, SWITCHES, _device, _profiled, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


def _takes_split(L, count: int, arm: str) -> bool:
    """The size 2 x 2 multiply of `count` items takes the head / middle / tail kernels (evaluator.cpp, the default build)."""
    logn = L.n.bit_length() - 1
    if arm == "whole" or not 12 <= logn <= 14:
        return False
    return arm == "split" or not (logn == 13 and count <= 16 or logn == 14 and count <= 4)


def _arm(L, monkeypatch, arm: str):
    """split: the pipelines chosen by the parameters alone; by_count: a few items may take the whole-polynomial kernels (n = 8192
    and 16384); whole: the whole-polynomial multiply (behz_extend_kernel, tensor, behz_floor_sk_kernel) at any degree."""
    return _device(L, monkeypatch, {"HIPBFV_NO_SPLIT_MUL": "1"} if arm == "whole" else None, split=arm == "split")


def _ran_multiply(seen, split: bool, what):
    if not DEFAULT_ARMS:
        assert "mul_head" in seen or "behz_extend" in seen, (what, seen)
    elif split:
        assert seen.get("mul_head") == 1 and seen.get("mul_tail") == 1 and "behz_extend" not in seen, (what, seen)
    else:
        assert seen.get("behz_extend") == 1 and seen.get("tensor") == 1 and seen.get("behz_floor_sk") == 1 and "mul_head" not in seen, (what, seen)


def _products(L, key, a, b):
    """The oracle's multiply of every item, once per process."""
    return L.cached(("products", key), lambda: np.stack([L.o.multiply(a[i], b[i]) for i in range(len(a))]))


def _relinearized(L, key, prods):
    return L.cached(("relinearized", key), lambda: np.stack([L.o.relinearize(p, L.rk) for p in prods]))


# ---- F: the multiply head -----------------------------------------------------------------------------------------------------
HEAD_RUNS = [("P1", "split"), ("P1", "by_count"), ("P1", "whole"), ("P3", "split"), ("P3", "by_count"), ("P4", "split"), ("P5", "split"),
             ("P5", "by_count"), ("W2048", "split"), ("U1024", "split")]


@pytest.mark.parametrize("pid,arm", HEAD_RUNS, ids=[f"{p}-{a}" for p, a in HEAD_RUNS])
def test_multiply_with_r_mtilde_and_the_scaled_rows_on_their_edges(pid, arm, monkeypatch):
    """Four items: random-y times edge-y, edge-y times random-y, all-rows-at-q-1 times random-y, edge-y times all-rows-at-q-1; every
    polynomial of both factors has r_mtilde on its six edges (r_mtilde = 2^31 must be centred as -2^31: the other sign moves the
    extended value by q).  P1 / P3: all FP64 (P3 with the grid sums in the head); P4: K = 8; P5: the mixed extension (by_count:
    behz_extend_coeff_mixed in the whole-polynomial kernel); W2048: 60-bit primes, the integer extension; U1024: 30-bit rows below
    m~ beside 50-bit ones."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = LD.mtilde_case(L)
    ref = _products(L, "head", a, b)
    ctx, ev = _arm(L, monkeypatch, arm)
    out, seen = _profiled(ev, lambda: ev.multiply(to_device(a), to_device(b)))
    print(pid, arm, "multiply:", seen)
    _same(to_host(out), ref, (pid, arm, "crafted head operands"))
    ev.check()
    _ran_multiply(seen, _takes_split(L, len(a), arm), (pid, arm))


@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_square_with_r_mtilde_on_its_edges(pid, monkeypatch):
    """multiply(a, a) on one device array: the head extends a once, the packed squaring middle kernel transforms it once."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = LD.mtilde_case(L)
    sq = np.ascontiguousarray(np.concatenate([a[:2], b[:2]]))  # random-y, edge-y, edge-y, random-y
    ref = _products(L, "square", sq, sq)
    ctx, ev = _arm(L, monkeypatch, "split")
    d = to_device(sq)
    out, seen = _profiled(ev, lambda: ev.multiply(d, d))
    _same(to_host(out), ref, (pid, "square"))
    ev.check()
    _ran_multiply(seen, True, (pid, "square"))


def test_a_3_by_2_product_with_r_mtilde_on_its_edges(monkeypatch):
    """Sizes other than 2 x 2 leave the split path: behz_extend_kernel over five polynomials, the floor over four."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing("P1")
    a, b = LD.mtilde_case(L, 3, 2, 2)
    ref = _products(L, "3 x 2", a, b)
    assert ref.shape[1] == 4
    ctx, ev = _arm(L, monkeypatch, "split")
    out, seen = _profiled(ev, lambda: ev.multiply(to_device(a), to_device(b)))
    _same(to_host(out), ref, "3 x 2")
    ev.check()
    _ran_multiply(seen, False, "3 x 2")


@pytest.mark.parametrize("pid", ["P3", "P5"])
def test_multiply_relin_with_r_mtilde_on_its_edges(pid, monkeypatch):
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = LD.mtilde_case(L)
    ref = _relinearized(L, "head", _products(L, "head", a, b))
    ctx, ev = _arm(L, monkeypatch, "split")
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    out, seen = _profiled(ev, lambda: ev.multiply_relin(to_device(a), to_device(b), rkd))
    print(pid, "multiply_relin:", seen)
    _same(to_host(out), ref, (pid, "multiply_relin"))
    ev.check()
    assert "ks_tail" in seen or "ks_moddown" in seen, seen
    if DEFAULT_ARMS:  # the fused pipeline: the product's c0 and c1 are formed in the key switch's last kernel
        assert seen.get("mul_head") == 1 and seen.get("ks_head") == 1 and seen.get("ks_tail") == 1 and "mul_tail" not in seen, seen


def test_multiply_sum_with_r_mtilde_on_its_edges(monkeypatch):
    """Three terms per group at P3: the head of the batched sum of products reads the crafted operands."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing("P3")
    a, b = LD.mtilde_case(L)
    prods = _products(L, "head", a, b)
    order = np.array([[0, 1, 2], [3, 2, 1]])
    ref = L.cached("head sums", lambda: np.stack([L.o.add(L.o.add(prods[g[0]], prods[g[1]]), prods[g[2]]) for g in order]))
    ctx, ev = _arm(L, monkeypatch, "split")
    out, seen = _profiled(ev, lambda: ev.multiply_sum(to_device(np.ascontiguousarray(a[order])), to_device(np.ascontiguousarray(b[order]))))
    _same(to_host(out), ref, "multiply_sum of crafted head operands")
    ev.check()
    if DEFAULT_ARMS:
        assert seen.get("mul_head") == 1 and seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen, seen


def test_two_products_of_a_program_read_crafted_operands(monkeypatch):
    """Two multiply + relinearize nodes in one program at P3: one merged launch whose head reads each member's operands where they
    are (MemberHead)."""
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.program import FheProgram

    L = landing("P3")
    a, b = LD.mtilde_case(L)
    p = FheProgram()
    ins = [p.append_input_ciphertext(i) for i in range(4)]
    p.append_output_ciphertext(p.append_relinearize(p.append_multiply(ins[0], ins[1])))
    p.append_output_ciphertext(p.append_relinearize(p.append_multiply(ins[2], ins[3])))
    desc = p.describe()
    print(desc)
    assert desc[0].startswith("mul_relin members=2"), desc
    # input sets: (a_i, b_i, b_j, a_j) over the four items
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0)]
    inputs = [np.stack([a[i] for i, j in pairs]), np.stack([b[i] for i, j in pairs]), np.stack([b[j] for i, j in pairs]), np.stack([a[j] for i, j in pairs])]
    ref = L.cached("program reference", lambda: [run_program(LD.MemoOracle(L.o), p.nodes, p.edges, [x[s] for x in inputs], L.rk) for s in range(len(pairs))])
    ctx, ev = _arm(L, monkeypatch, "split")
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    got, seen = _profiled(ev, lambda: [to_host(t) for t in p.run(ev, [to_device(x) for x in inputs], rkd)])
    print("two products:", seen)
    for k in range(2):
        _same(got[k], np.stack([ref[s][k] for s in range(len(pairs))]), ("two products", k))
    ev.check()
    if DEFAULT_ARMS:
        assert seen.get("mul_head") == 1 and seen.get("ks_tail") == 1 and "mul_tail" not in seen, seen  # both members in one launch


# ---- G: the floor's inputs and the multiply's outputs -------------------------------------------------------------------------
def _floor_operands(L):
    """Four items times (1, 1): y on the edge cycle, every row at q - 1 / 0, and the two harvested operands."""
    return L.cached("floor operands", lambda: (np.ascontiguousarray(np.concatenate([LD.floor_case(L)[0], LD.output_case(L)[0]])), LD.ones_ct(L, 4)))


FLOOR_RUNS = [("P1", "split"), ("P1", "by_count"), ("P1", "whole"), ("P3", "split"), ("P3", "by_count"), ("P4", "split"), ("P5", "split"),
              ("P5", "by_count"), ("W2048", "split")]


@pytest.mark.parametrize("pid,arm", FLOOR_RUNS, ids=[f"{p}-{a}" for p, a in FLOOR_RUNS])
def test_multiply_by_one_one_puts_the_floor_inputs_and_the_outputs_on_their_edges(pid, arm, monkeypatch):
    """a (1, 1) = (a0, a0 + a1, a1): items 0 and 1 hand the floor y_i = t d (q / q_i)^-1 on 0, q_i - 1, 1, (q_i -+ 1) / 2 and on
    q_i - 1 in all rows at once (a y_i of q_i in place of 0 moves the floor by one); items 2 and 3 come out as 0, q_i - 1 and 1 in
    every row of polynomials 0 and 2."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = _floor_operands(L)
    ref = _products(L, "floor", a, b)
    kinds = LD.output_case(L)[1]
    for i in range(2):  # (what tests/test_landing_cpu.py shows: the reference IS the target)
        assert (ref[2 + i][0] == LD.kinds_to_words(L.primes, kinds[i, 0])).all() and (ref[2 + i][2] == LD.kinds_to_words(L.primes, kinds[i, 1])).all()
    ctx, ev = _arm(L, monkeypatch, arm)
    out, seen = _profiled(ev, lambda: ev.multiply(to_device(a), to_device(b)))
    print(pid, arm, "multiply by (1, 1):", seen)
    _same(to_host(out), ref, (pid, arm, "floor inputs and outputs"))
    ev.check()
    _ran_multiply(seen, _takes_split(L, len(a), arm), (pid, arm))


@pytest.mark.parametrize("pid", ["P1", "P3", "P4", "P5"])
def test_multiply_relin_by_one_one_on_the_edges(pid, monkeypatch):
    """mulrelin_head floors d2 = a1 into the key switch's digits, mulrelin_tail floors d0 and d1: the landed y and the landed outputs
    of d2 are what the digit decomposition reads."""
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = _floor_operands(L)
    ref = _relinearized(L, "floor", _products(L, "floor", a, b))
    ctx, ev = _arm(L, monkeypatch, "split")
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    out, seen = _profiled(ev, lambda: ev.multiply_relin(to_device(a), to_device(b), rkd))
    print(pid, "multiply_relin by (1, 1):", seen)
    _same(to_host(out), ref, (pid, "multiply_relin by (1, 1)"))
    ev.check()
    assert "ks_tail" in seen or "ks_moddown" in seen, seen
    if DEFAULT_ARMS:
        assert seen.get("mul_head") == 1 and seen.get("ks_head") == 1 and seen.get("ks_tail") == 1 and "mul_tail" not in seen, seen


@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_sums_of_products_pass_through_q_minus_1(pid, monkeypatch):
    """Three terms whose outputs are 0, q_i - 1, q_i - 1 in some order in every coefficient of polynomials 0 and 2: the sums of
    canonical residues in mul_tail_sum_kernel pass through q_i - 1 and wrap to q_i - 2 (P4: the arm that adds through the output
    rows).  multiply_sum and multiply_sum_relin."""
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, kinds = LD.output_sum_case(L)
    groups, terms = a.shape[:2]
    b = LD.ones_ct(L, groups * terms).reshape(a.shape)

    def make():
        sums = []
        for g in range(groups):
            acc = None
            for j in range(terms):
                term = L.o.multiply(a[g, j], b[g, j])
                acc = term if acc is None else L.o.add(acc, term)
            sums.append(acc)
        return np.stack(sums), np.stack([L.o.relinearize(s, L.rk) for s in sums])

    ref3, ref2 = L.cached("output sums reference", make)
    qm2 = np.array(L.primes, dtype=np.uint64)[:, None] - 2
    assert (ref3[:, 0] == qm2).all() and (ref3[:, 2] == qm2).all()
    ctx, ev = _arm(L, monkeypatch, "split")
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    da, db = to_device(a), to_device(b)
    out3, seen = _profiled(ev, lambda: ev.multiply_sum(da, db))
    print(pid, "multiply_sum:", seen)
    _same(to_host(out3), ref3, (pid, "multiply_sum"))
    if DEFAULT_ARMS:
        assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "eltwise" not in seen, seen
    out2, seen = _profiled(ev, lambda: ev.multiply_sum_relin(da, db, rkd))
    _same(to_host(out2), ref2, (pid, "multiply_sum_relin"))
    ev.check()
    if DEFAULT_ARMS:
        assert seen.get("mul_tail_sum") == 1 and "ks_tail" in seen, seen


# ---- H: decrypt's gamma correction --------------------------------------------------------------------------------------------
GAMMA_CASES = [(p, t) for p in ("P1", "P2", "P3", "W4096") for t in (None, 500, (1 << 60) - 1)]


def _gamma_reference(L, size):
    def make():
        ct = LD.gamma_case(L, 2, size)[0]
        return np.stack([L.o.decrypt(c, L.sk) for c in ct]), [L.o.noise_budget(c, L.sk) for c in ct]

    return L.cached(("gamma reference", size), make)


def _decrypt_three_ways(L, size, monkeypatch, what):
    from sunscreen_amd import SecretKey
    from sunscreen_amd.batch import to_device, to_host

    ct = LD.gamma_case(L, 2, size)[0]
    ref, budgets = _gamma_reference(L, size)
    ctx, ev = _device(L, monkeypatch)
    skd = SecretKey.from_array(ctx, L.sk)
    d = to_device(ct)
    out, seen = _profiled(ev, lambda: ev.decrypt(d, skd))
    assert seen.get("ntt_fwd") == 1 and seen.get("ntt_inv") == 1, seen
    _same(to_host(out), ref, (what, "decrypt"))
    (plain, budget), seen = _profiled(ev, lambda: ev.decrypt_checked(d, skd))
    assert seen.get("ntt_fwd") == 1 and seen.get("ntt_inv") == 1, seen
    _same(to_host(plain), ref, (what, "decrypt_checked"))
    assert [int(v) for v in budget.cpu()] == budgets, (what, "decrypt_checked budget")
    assert [int(v) for v in ev.noise_budget(d, skd).cpu()] == budgets, (what, "noise_budget")


@pytest.mark.parametrize("pid,t", GAMMA_CASES, ids=[f"{p}-t{t or 'batching'}" for p, t in GAMMA_CASES])
def test_decrypt_with_the_gamma_residue_on_its_edges(pid, t, monkeypatch):
    """decrypt, decrypt_checked and noise_budget on ciphertexts whose gamma residue g is 0, 1, floor(gamma / 2) - 1, floor(gamma / 2),
    floor(gamma / 2) + 1 and gamma - 1, cycled over the coefficients (g = floor(gamma / 2) is NOT above gamma / 2: the other branch
    moves the plaintext by one).  A batching t, a small raw t and t = 2^60 - 1, above every data prime."""
    _decrypt_three_ways(landing(pid, t), 2, monkeypatch, (pid, t))


def test_decrypt_a_size_3_ciphertext_with_the_gamma_residue_on_its_edges(monkeypatch):
    """The crafted phase in c0, random c1 and c2."""
    _decrypt_three_ways(landing("P1"), 3, monkeypatch, ("P1", "size 3"))
