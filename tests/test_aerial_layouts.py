"""The Aerial preprocessing oracle (oracle/pe_ref.aerial_nn_indices / aerial_preprocess) over the
DMRS layouts nrx_forward_aerial accepts, against a brute-force restatement: plain loops, no argmin,
no meshgrid, a direct mean / population std.  tests/test_gpu_aerial_contract.py compares the GPU
preprocessing with the oracle over the same table, so what is pinned here is its reference.

LAYOUTS: name -> (dmrs_ofdm_pos rows, dmrs_subcarrier_pos rows), one row per user.
  type1_2sym          the nrx_rt layout: type-1 combs in CDM-group order on symbols (2, 11)
  one_sym_u3          one DMRS symbol, three users
  three_sym_per_user  three symbols, different per user
  type2_npil4         type-2-like adjacent pairs, four pilots per PRB, three groups
  npil2_edges         two pilots per PRB on the first and last symbol: distances up to 6 + 10
  descending          non-ascending position lists: the first minimum follows the list order
  four_sym            four symbols
  all_pilots          every RE a pilot: both PE components have std == 0 and are exactly 0
  all_sc_one_sym      every subcarrier of one symbol: the frequency component has std == 0
"""
import numpy as np
import pytest

from oracle import pe_ref
from tests.test_aerial import _oracle_gather_direct

T = 14
EVENS = (0, 2, 4, 6, 8, 10)
ODDS = (1, 3, 5, 7, 9, 11)
LAYOUTS = {
    "type1_2sym": ([(2, 11)] * 2, [EVENS, ODDS]),
    "one_sym_u3": ([(3,)] * 3, [ODDS, EVENS, ODDS]),
    "three_sym_per_user": ([(2, 7, 11), (0, 5, 10)], [EVENS, ODDS]),
    "type2_npil4": ([(2, 11)] * 3, [(0, 1, 6, 7), (2, 3, 8, 9), (4, 5, 10, 11)]),
    "npil2_edges": ([(0, 13)], [(0, 1)]),
    "descending": ([(11, 2)], [(10, 8, 6, 4, 2, 0)]),
    "four_sym": ([(2, 5, 8, 11)], [EVENS]),
    "all_pilots": ([tuple(range(14))], [tuple(range(12))]),
    "all_sc_one_sym": ([(6,)], [tuple(range(12))]),
}


def layout_positions(name, users=None):
    """(dmrs_ofdm_pos [U, nsym], dmrs_subcarrier_pos [U, npil]) int32; ``users``: the rows of the
    layout repeated in turn over that many users."""
    ofdm, scp = LAYOUTS[name]
    U = users or len(ofdm)
    return (np.array([ofdm[u % len(ofdm)] for u in range(U)], np.int32),
            np.array([scp[u % len(scp)] for u in range(U)], np.int32))


def aerial_inputs(name, B, F, A, seed, users=None):
    """iid standard normal y_* / h_ls_* (neighbouring pilots differ by O(1): a gather from the
    wrong pilot pair cannot hide) and the layout's positions, as the nrx_aerial_io feed dict."""
    ofdm, scp = layout_positions(name, users)
    U, nsym, npil = ofdm.shape[0], ofdm.shape[1], scp.shape[1]
    rng = np.random.default_rng(seed)
    yr, yi = rng.standard_normal((2, B, F, T, A)).astype(np.float32)
    hr, hi = rng.standard_normal((2, B, nsym * (F // 12) * npil, U, A)).astype(np.float32)
    return dict(y_real=yr, y_imag=yi, h_ls_real=hr, h_ls_imag=hi, dmrs_ofdm_pos=ofdm, dmrs_subcarrier_pos=scp)


def within_one_ulp(got, want):
    """|got - want| <= one float32 ulp of want, and got == want where want == 0."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    ulp = np.where(want == 0, np.float32(0), np.spacing(np.abs(want)))
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all())


def brute_force_tables(ofdm, scp, nprb):
    """nn [U, T, 12]: the first pilot in (symbol, pilot) list order at minimal Manhattan distance;
    pe [U, 12 nprb, T, 2]: minimal |t - t_k| and |sc - sc_j|, each minus its mean over the 12 x T
    REs of a PRB and divided by the population std where that is > 0, repeated over PRBs."""
    U, nsym, npil = ofdm.shape[0], ofdm.shape[1], scp.shape[1]
    nn = np.zeros((U, T, 12), np.int64)
    pe = np.zeros((U, 12 * nprb, T, 2), np.float64)
    for u in range(U):
        dist = np.zeros((2, T, 12))
        for t in range(T):
            for sc in range(12):
                best, bestd = -1, None
                for k in range(nsym):
                    for j in range(npil):
                        d = abs(t - int(ofdm[u, k])) + abs(sc - int(scp[u, j]))
                        if bestd is None or d < bestd:
                            best, bestd = k * npil + j, d
                nn[u, t, sc] = best
                dist[0, t, sc] = min(abs(t - int(ofdm[u, k])) for k in range(nsym))
                dist[1, t, sc] = min(abs(sc - int(scp[u, j])) for j in range(npil))
        for c in range(2):
            vals = [float(v) for v in dist[c].ravel()]
            mean = sum(vals) / len(vals)
            std = (sum((v - mean) ** 2 for v in vals) / len(vals)) ** 0.5
            for t in range(T):
                for sc in range(12):
                    v = dist[c, t, sc] - mean
                    for prb in range(nprb):
                        pe[u, prb * 12 + sc, t, c] = v / std if std > 0 else v
    return nn, pe.astype(np.float32)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_oracle_tables_match_brute_force(name):
    ofdm, scp = layout_positions(name)
    nn, pe = pe_ref.aerial_nn_indices(ofdm, scp, T, 2)
    bnn, bpe = brute_force_tables(ofdm, scp, 2)
    U = ofdm.shape[0]
    assert nn.shape == (U, 1, T, 12) and pe.shape == (U, 24, T, 2) and pe.dtype == np.float32
    np.testing.assert_array_equal(nn[:, 0], bnn)
    assert nn.min() >= 0 and nn.max() < ofdm.shape[1] * scp.shape[1]
    # both in f64, rounded once to f32; only the order of the sums differs
    assert within_one_ulp(pe, bpe), np.abs(pe - bpe).max()
    if name == "all_pilots":
        assert not pe.any()
    if name == "all_sc_one_sym":
        assert not pe[..., 1].any() and pe[..., 0].any()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_oracle_preprocess_matches_direct_gather(name):
    B, F, A = 2, 24, 3
    x = aerial_inputs(name, B, F, A, seed=7)
    ofdm, scp = x["dmrs_ofdm_pos"], x["dmrs_subcarrier_pos"]
    U, nsym, npil = ofdm.shape[0], ofdm.shape[1], scp.shape[1]
    y, h, pe = pe_ref.aerial_preprocess(x["y_real"], x["y_imag"], x["h_ls_real"], x["h_ls_imag"], ofdm, scp, U)
    np.testing.assert_array_equal(y, np.concatenate([x["y_real"], x["y_imag"]], -1))
    bnn, bpe = brute_force_tables(ofdm, scp, F // 12)
    want = _oracle_gather_direct(x["h_ls_real"], x["h_ls_imag"], bnn[:, None], B, U, F, T, A, nsym, npil)
    assert h.dtype == np.float32
    np.testing.assert_array_equal(h, want)
    assert within_one_ulp(pe, bpe)


def test_layout_table_reaches_what_it_claims():
    # ties between pilots of different FOCC pairs and of different symbols exist in the table (a
    # last-minimum tie-break changes nn, and the gathered pair, on such REs)
    cross_pair = cross_sym = 0
    for name in LAYOUTS:
        ofdm, scp = layout_positions(name)
        npil = scp.shape[1]
        for u in range(ofdm.shape[0]):
            for t in range(T):
                for sc in range(12):
                    d = [abs(t - int(a)) + abs(sc - int(b)) for a in ofdm[u] for b in scp[u]]
                    ties = [i for i, v in enumerate(d) if v == min(d)]
                    cross_pair += any(i // 2 != ties[0] // 2 for i in ties)
                    cross_sym += any(i // npil != ties[0] // npil for i in ties)
    assert cross_pair > 0 and cross_sym > 0
    assert within_one_ulp([1.0, 0.0], [1.0 + 2.0 ** -23, 0.0])
    assert not within_one_ulp([1.0], [1.0 + 2.0 ** -22]) and not within_one_ulp([1e-30], [0.0])
