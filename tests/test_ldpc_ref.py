"""The numpy oracle of the QC-LDPC decoder (tests/ldpc_ref.py) and the code construction
(neural_rx_amd/ldpc.py), on the CPU: the symmetry the coded evaluation rests on, the properties of
the constructed codes and of the committed tables, and a waterfall sanity point."""
import json

import numpy as np
import pytest

from neural_rx_amd import ldpc
from tests import ldpc_ref as R


def _null_space_gf2(H):
    """rows: a basis of {c : H c = 0} over GF(2)"""
    H = H.copy() % 2
    m, n = H.shape
    piv, r = [], 0
    for c in range(n):
        rows = np.nonzero(H[r:, c])[0]
        if not len(rows):
            continue
        H[[r, r + rows[0]]] = H[[r + rows[0], r]]
        for i in np.nonzero(H[:, c])[0]:
            if i != r:
                H[i] ^= H[r]
        piv.append(c)
        r += 1
        if r == m:
            break
    free = [c for c in range(n) if c not in piv]
    basis = np.zeros((len(free), n), np.uint8)
    for k, f in enumerate(free):
        basis[k, f] = 1
        for i, pc in enumerate(piv):
            basis[k, pc] = H[i, f]
    return basis


@pytest.fixture(scope="module")
def tiny():
    return ldpc.make_regular_qc(2, 4, 8, 8, seed=3)


@pytest.mark.parametrize("cn_type", [0, 1])
def test_symmetry_all_zero_word_under_a_scrambler(tiny, cn_type):
    """Decoding a random codeword c from noisy LLRs equals decoding the all-zero word from the
    sign-flipped LLRs, XOR c, bit for bit: the decoder is sign-symmetric (boxplus and min-sum are odd
    in every argument, the clamps are symmetric), which is what lets the evaluation decode the
    descrambled LLRs of uncoded random bits towards zero."""
    H = R.parity_matrix(tiny)
    basis = _null_space_gf2(H)
    assert len(basis) >= tiny.n - tiny.mb * tiny.z and not ((H.astype(int) @ basis.T.astype(int)) % 2).any()
    rng = np.random.RandomState(11)
    n = 24
    c = (rng.randint(0, 2, (n, len(basis))) @ basis % 2).astype(np.uint8)
    assert c.any() and not ((H.astype(int) @ c.T.astype(int)) % 2).any()
    sigma2 = 0.7
    y = (1.0 - 2.0 * c) + np.sqrt(sigma2) * rng.standard_normal(c.shape)
    l = (2.0 * y / sigma2).astype(np.float32)
    flipped = (l * (1.0 - 2.0 * c)).astype(np.float32)
    for early in (False, True):
        a = R.decode(tiny, l, 6, cn_type, 0.75, early)
        z = R.decode(tiny, flipped, 6, cn_type, 0.75, early)
        assert np.array_equal(a["hard"], z["hard"] ^ c)
        assert np.array_equal(a["iters"], z["iters"]) and np.array_equal(a["parity_ok"], z["parity_ok"])
        assert np.array_equal(np.abs(a["app"]), np.abs(z["app"]))
    assert 0 < a["parity_ok"].sum()                    # the point is neither trivial nor hopeless
    assert (z["hard"].any(axis=1)).sum() > 0


def test_parity_ok_is_the_syndrome_of_hard(tiny):
    """pins the edge convention: check i z + r, variable j z + (r + s) mod z"""
    H = R.parity_matrix(tiny).astype(int)
    l = R.awgn_llrs(40, tiny.n, 2.0, 0.5, 5)
    o = R.decode(tiny, l, 3)
    syn = (H @ o["hard"].T.astype(int)) % 2
    assert np.array_equal(o["parity_ok"], (~syn.any(axis=0)).astype(np.uint8))
    assert 0 < o["parity_ok"].sum() < 40
    # a tie decides 1: an all-erased input never passes as the all-zero word
    e = R.decode(tiny, np.zeros((1, tiny.n), np.float32), 2)
    assert e["hard"].all() and not e["app"].any()


@pytest.mark.parametrize("name", sorted(ldpc.NAMED))
def test_construction(name):
    dv, dc, nb = ldpc.NAMED[name]
    z = 24
    c = ldpc.make_regular_qc(dv, dc, nb, z, seed=5)
    on = c.shifts >= 0
    assert c.mb == nb * dv // dc and c.kb == nb - c.mb and c.shifts.shape == (c.mb, nb)
    assert (on.sum(0) == dv).all() and (on.sum(1) == dc).all()
    assert c.shifts.max() < z and c.shifts.min() >= -1
    assert not ldpc.has_4cycle(c.shifts, z)
    assert np.array_equal(c.shifts, ldpc.make_regular_qc(dv, dc, nb, z, seed=5).shifts)
    assert not np.array_equal(c.shifts, ldpc.make_regular_qc(dv, dc, nb, z, seed=6).shifts)


def test_has_4cycle_sees_one():
    s = np.array([[0, 0, -1], [1, 1, 0]], np.int16)    # columns 0 and 1 share both rows, difference 0
    assert ldpc.has_4cycle(s, 8)
    s[1, 1] = 2
    assert not ldpc.has_4cycle(s, 8)


def test_committed_tables_regenerate():
    with open(ldpc.TABLES, encoding="utf-8") as f:
        tables = json.load(f)
    assert set(tables) == {"r12_z96", "r23_z64", "r34_z96", "r13_z96"}
    for key, t in tables.items():
        name, z = key.split("_z")
        dv, dc, nb = ldpc.NAMED[name]
        c = ldpc.make_regular_qc(dv, dc, nb, int(z), t["seed"])
        assert (c.mb, c.nb, c.z, c.kb) == (t["mb"], t["nb"], t["z"], t["kb"])
        assert c.shifts.tolist() == t["shifts"]
        assert np.array_equal(ldpc.named_code(name, int(z)).shifts, c.shifts)
        assert not ldpc.has_4cycle(c.shifts, c.z)


def test_fit():
    code, C = ldpc.fit("r12", 2304)                    # nrx_rt, 4 PRB, 16-QAM
    assert (C, code.z, code.n, code.num_info, code.rate) == (1, 96, 2304, 1152, 0.5)
    code, C = ldpc.fit("r23", 2304)
    assert (C, code.z, code.rate) == (1, 64, 24 / 36)
    code, C = ldpc.fit("r12", 24 * 384 + 100)          # one codeword too many bits: two, with left-over bits
    assert C == 2 and code.z == (24 * 384 + 100) // 48
    with pytest.raises(ValueError):
        ldpc.fit("r12", 40)


def test_waterfall_sanity():
    """r12 at z = 96, seeded BPSK-AWGN LLRs at Eb/N0 3.5 dB: 64 of 64 decode with parity_ok in at most 8
    iterations (a float64 prototype of the schedule measured 512 of 512 with a maximum of 4)."""
    code = ldpc.named_code("r12", 96)
    o = R.decode(code, R.awgn_llrs(64, code.n, 3.5, 0.5, 7), 20, early_stop=True)
    print("iterations", np.bincount(o["iters"]))
    assert o["parity_ok"].all() and o["iters"].max() <= 8 and not o["hard"].any()
