"""The GPU QC-LDPC decoder and its slot glue (nrx_ldpc_decode / nrx_ldpc_gather / nrx_ldpc_count,
include/nrx.h) against the float64 numpy oracle of tests/ldpc_ref.py (needs an MI355X).

Tolerance of the ``app`` comparisons (D1, D2, D4, D6).  The kernel runs the oracle's schedule in f32
with the device's ``expf`` / ``log1pf``.  For every case the test runs the same schedule on the same
inputs in f32 numpy and takes the largest |f32 - f64| difference of ``app``; the gate is 4 times that
(the factor covers the device's transcendental functions, a few ulp against numpy's).  Measured on
the CPU for the inputs below, largest |f32 - f64|, boxplus / min-sum:
    D1 (4 x 8, z 8, 33 codewords)         1 iteration 1.04e-06 / 1.11e-06    2 iterations 2.03e-06 / 1.85e-06
    D2 (5 x 11 irregular, z 13, 45)       1 iteration 1.33e-06 / 1.29e-06    2 iterations 2.48e-06 / 3.19e-06
    D4 (46 x 68, 2 iterations)            z 384, 2 codewords 5.50e-06 / 5.77e-06    z 8, 40 codewords 2.53e-06 / 7.90e-06
so the gates lie between 4.2e-06 and 3.2e-05, on values of up to 18 (one f32 ulp there is 1.9e-06); the
test computes them again, so they follow the inputs.  ``hard`` must be equal wherever |app| of the oracle
exceeds the gate.
"""
import functools

import numpy as np
import pytest

from neural_rx_amd import ldpc
from tests import ldpc_ref as R

pytestmark = pytest.mark.gpu


def _gpu_decode(code, llr, num_iter, cn_type=0, ms_scale=0.75, early_stop=False, skip=None, want_app=True,
                decoder=None):
    import torch
    dec = decoder or ldpc.Decoder(code)
    t = torch.from_numpy(np.ascontiguousarray(llr, np.float32)).cuda()
    sk = torch.from_numpy(np.ascontiguousarray(skip, np.uint8)).cuda() if skip is not None else None
    out = dec.decode(t, num_iter, cn_type, ms_scale, early_stop, 20.0, skip=sk, want_app=want_app)
    torch.cuda.synchronize()
    res = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
    res["workspace_bytes"] = dec.last_workspace_bytes
    return res


def _gate(code, llr, num_iter, cn_type, ms_scale=0.75, skip=None):
    """(oracle, tolerance): 4 x the largest |f32 numpy - f64 numpy| app difference on these inputs"""
    ref = R.decode(code, llr, num_iter, cn_type, ms_scale, False, skip=skip)
    f32 = R.decode(code, llr, num_iter, cn_type, ms_scale, False, skip=skip, dtype=np.float32)
    d = float(np.abs(f32["app"].astype(np.float64) - ref["app"]).max())
    assert 0 < d < 1e-4
    return ref, 4.0 * d


def _check_app(got, ref, tol, label):
    err = float(np.abs(got["app"].astype(np.float64) - ref["app"]).max())
    print(f"{label}: max |app - oracle| {err:.3e}  gate {tol:.3e}  max |app| {np.abs(ref['app']).max():.1f}")
    assert np.isfinite(got["app"]).all()
    assert err <= tol
    firm = np.abs(ref["app"]) > tol
    assert np.array_equal(got["hard"][firm], ref["hard"][firm])
    assert np.array_equal(got["iters"], ref["iters"])
    # parity_ok is a function of hard: compare where no decision of the codeword is within the gate of 0
    sure = firm.all(axis=1)
    assert np.array_equal(got["parity_ok"][sure], ref["parity_ok"][sure])


@functools.lru_cache(maxsize=None)
def _tiny():
    return ldpc.make_regular_qc(2, 4, 8, 8, seed=3)


@functools.lru_cache(maxsize=None)
def _irregular():
    """5 x 11 at z = 13: row weights 2, 3, 5, 6, 7, column 10 of weight 1, -1 entries everywhere else"""
    rng = np.random.RandomState(21)
    s = np.full((5, 11), -1, np.int16)
    rows = {0: [0, 1], 1: [2, 3, 4], 2: [0, 5, 6, 7, 8], 3: [1, 2, 5, 6, 8, 9], 4: [0, 3, 4, 7, 8, 9, 10]}
    for i, cols in rows.items():
        s[i, cols] = rng.randint(0, 13, len(cols))
    w = (s >= 0).sum(1)
    assert list(w) == [2, 3, 5, 6, 7] and ((s >= 0).sum(0) >= 1).all() and (s >= 0)[:, 10].sum() == 1
    return ldpc.QCCode(5, 11, 13, 6, s)


@functools.lru_cache(maxsize=None)
def _limits(z):
    """46 x 68 with row weights 3..19 and random shifts, no girth search: not a TS 38.212 table"""
    rng = np.random.RandomState(4)
    s = np.full((46, 68), -1, np.int16)
    for i in range(46):
        cols = rng.permutation(68)[:3 + i % 17]
        s[i, cols] = rng.randint(0, z, len(cols))
    s[0, s.max(0) < 0] = 1
    assert (s >= 0).sum(1).max() == 19 and ((s >= 0).sum(0) >= 1).all()
    return ldpc.QCCode(46, 68, z, 22, s)


@pytest.mark.parametrize("cn_type", [0, 1])
@pytest.mark.parametrize("num_iter", [1, 2])
def test_d1_tiny_code(num_iter, cn_type):
    """D1: 4 x 8, z = 8 (32 codewords per workgroup: 33 codewords are two workgroups)"""
    code = _tiny()
    llr = R.awgn_llrs(33, code.n, 1.0, 0.5, 3)
    ref, tol = _gate(code, llr, num_iter, cn_type)
    got = _gpu_decode(code, llr, num_iter, cn_type)
    _check_app(got, ref, tol, f"D1 it {num_iter} cn {cn_type}")
    assert got["workspace_bytes"] == 256               # the messages are in LDS


@pytest.mark.parametrize("cn_type", [0, 1])
@pytest.mark.parametrize("num_iter", [1, 2])
def test_d2_odd_z_irregular(num_iter, cn_type):
    """D2: z = 13, a partial wave per codeword, 19 codewords per workgroup, the last workgroup partial"""
    code = _irregular()
    llr = R.awgn_llrs(45, code.n, 1.0, 0.5, 4)
    ref, tol = _gate(code, llr, num_iter, cn_type)
    got = _gpu_decode(code, llr, num_iter, cn_type)
    _check_app(got, ref, tol, f"D2 it {num_iter} cn {cn_type}")


@functools.lru_cache(maxsize=None)
def _r12():
    code = ldpc.named_code("r12", 96)
    return code, ldpc.Decoder(code)


def test_d3_r12_waterfall():
    """D3: r12 at z = 96 (two codewords per workgroup), 20 iterations with early stop.  Near threshold
    f32 and f64 BP may part: at most 2 of 64 codewords may differ at 1.5 dB (the f32 numpy oracle
    differed from the f64 one on 0 of 5120).  At 3.5 dB all 64 come out all-zero with parity_ok."""
    code, dec = _r12()
    llr = R.awgn_llrs(64, code.n, 1.5, 0.5, 7)
    ref = R.decode(code, llr, 20, early_stop=True)
    got = _gpu_decode(code, llr, 20, early_stop=True, want_app=False, decoder=dec)
    blk = lambda o: o["hard"][:, :code.num_info].any(axis=1)   # noqa: E731
    differ = (got["iters"] != ref["iters"]) | (got["parity_ok"] != ref["parity_ok"]) | (blk(got) != blk(ref))
    print(f"D3 1.5 dB: block errors {blk(got).sum()} (oracle {blk(ref).sum()})  iterations {np.bincount(got['iters'])}  "
          f"codewords that differ {differ.sum()}")
    assert differ.sum() <= 2
    assert 0 < blk(ref).sum() < 64
    got = _gpu_decode(code, R.awgn_llrs(64, code.n, 3.5, 0.5, 7), 20, early_stop=True, want_app=False, decoder=dec)
    assert got["parity_ok"].all() and not got["hard"].any() and got["iters"].max() <= 8


@pytest.mark.parametrize("cn_type", [0, 1])
@pytest.mark.parametrize("z,num_cw", [(384, 2), (8, 40)])
def test_d4_size_limits_messages_in_workspace(z, num_cw, cn_type):
    """D4: mb 46, nb 68: at z = 384 APP alone takes 102 KiB of LDS and the messages of one codeword go
    to the workspace; at z = 8 the same base runs 32 codewords per workgroup on that path"""
    code = _limits(z)
    llr = R.awgn_llrs(num_cw, code.n, 1.0, 22 / 68, 5)
    ref, tol = _gate(code, llr, 2, cn_type)
    got = _gpu_decode(code, llr, 2, cn_type)
    _check_app(got, ref, tol, f"D4 z {z} cn {cn_type}")
    assert got["workspace_bytes"] == num_cw * int((code.shifts >= 0).sum()) * z * 4


def test_d5_deterministic_and_split_independent():
    import torch
    code, dec = _r12()
    llr = torch.from_numpy(R.awgn_llrs(64, code.n, 1.5, 0.5, 9)).cuda()
    runs = []
    for _ in range(2):
        o = dec.decode(llr, 20, early_stop=True, want_app=True)
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy().copy() for k, v in o.items()})
    halves = []
    for part in (llr[:32].contiguous(), llr[32:].contiguous()):
        o = dec.decode(part, 20, early_stop=True, want_app=True)
        torch.cuda.synchronize()
        halves.append({k: v.cpu().numpy().copy() for k, v in o.items()})
    for k in ("hard", "app", "iters", "parity_ok"):
        assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k
        both = np.concatenate([halves[0][k], halves[1][k]])
        assert np.array_equal(runs[0][k].view(np.uint8), both.view(np.uint8)), k
    assert 1 < runs[0]["iters"].min() and runs[0]["iters"].max() == 20


@pytest.mark.parametrize("cn_type", [0, 1])
def test_d6_skip_and_special_values(cn_type):
    code = _irregular()
    llr = R.awgn_llrs(45, code.n, 2.0, 0.5, 6)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30]
    rng = np.random.RandomState(2)
    for cw in range(0, 45, 2):
        at = rng.permutation(code.n)[:len(special)]
        llr[cw, at] = special
    llr[44] = 0.0                                      # all erased: never passes as the all-zero word
    skip = np.zeros(45, np.uint8)
    skip[[1, 18, 19, 43]] = 1
    ref, tol = _gate(code, llr, 2, cn_type, skip=skip)
    got = _gpu_decode(code, llr, 2, cn_type, skip=skip)
    _check_app(got, ref, tol, f"D6 cn {cn_type}")
    for k in ("hard", "app", "iters", "parity_ok"):
        assert not got[k][skip == 1].any(), k
    assert (got["iters"][skip == 0] == 2).all()
    assert got["hard"][44].all() and not got["parity_ok"][44] and not got["app"][44].any()
    es = _gpu_decode(code, llr, 20, cn_type, early_stop=True, skip=skip)
    rs = R.decode(code, llr, 20, cn_type, 0.75, True, skip=skip)
    assert np.isfinite(es["app"]).all() and not es["iters"][skip == 1].any()
    assert ((es["iters"] != rs["iters"]) | (es["parity_ok"] != rs["parity_ok"])).sum() <= 2


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("with_cols", [True, False])
def test_g1_gather_is_exact(heads, with_cols):
    """G1: B 2, U 3, F 13, one DMRS symbol, MCS from 2 / 4 / 6 bits, stride 6, slot 0 user 1 inactive,
    C = 2 with left-over bits (169 data REs: 338 / 676 / 1014 bits at 300 per codeword), a tx_col with
    repeats, unlisted columns and two entries outside 0..N-1, a col_prior; f32 sums in ascending e'"""
    import torch
    rng = np.random.RandomState(31 + heads)
    B, U, F, T, BS, C, n_tx, N = 2, 3, 13, 14, 6, 2, 300, 320
    mcs_bits, dmrs = [2, 4, 6], [3]
    llr = (rng.standard_normal((heads, B, U, F, T, BS)) * 7).astype(np.float32)
    bits = rng.randint(0, 2, (B, U, F, T, BS)).astype(np.uint8)
    mcs = np.array([[0, 1, 2], [2, 0, 1]], np.uint8)
    active = np.ones((B, U), np.float32)
    active[0, 1] = 0
    tx_col = col_prior = None
    if with_cols:
        tx_col = rng.randint(0, 300, n_tx).astype(np.int32)
        tx_col[7], tx_col[150] = -1, N
        tx_col[255], tx_col[256], tx_col[257] = 5, 5, 5   # a column repeated across and inside a chunk of 256
        col_prior = (rng.standard_normal(N) * 3).astype(np.float32)
        assert len(np.unique(tx_col)) < n_tx - 50
    want, want_skip = R.gather(llr, bits, mcs, active, mcs_bits, dmrs, C, n_tx, N, tx_col, col_prior)
    dev = lambda a: torch.from_numpy(a).cuda() if a is not None else None   # noqa: E731
    got, got_skip = ldpc.gather(dev(llr), dev(bits), dev(active), dev(mcs), mcs_bits, dmrs, C, n_tx, N, dev(tx_col),
                                dev(col_prior))
    torch.cuda.synchronize()
    assert list(want_skip) == [0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0]
    assert np.array_equal(got_skip.cpu().numpy(), want_skip)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_c1_count_is_exact_and_accumulates():
    import torch
    B, U, C, N, K = 3, 2, 2, 64, 40
    hard = np.zeros((B, U, C, N), np.uint8)
    skip = np.zeros((B, U, C), np.uint8)
    iters = np.full((B, U, C), 5, np.int32)
    hard[0, 0, 0, [1, 39]] = 1                         # two information-bit errors
    hard[0, 0, 1, [40, 63]] = 1                        # parity columns only: not counted
    hard[1, 0, 1, 0] = 7                               # any non-zero value is an error
    hard[1, 1, 0, :] = 1
    skip[1, 1, 0] = 1                                  # ... but this codeword is skipped
    skip[2, 1, :] = 1                                  # a (slot, user) without a codeword: no block
    hard[2, 0, 0, 3] = hard[2, 0, 1, 4] = 1            # two codewords of one block in error: one block error
    iters[2, 0, 1] = 20
    want, want_it = R.count(hard, skip, B, U, C, K, iters)
    assert want.tolist() == [[5, 6 * K, 3, 3], [0, 3 * K, 0, 2]] and want_it.tolist() == [[45, 6], [15, 3]]
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    counts = torch.zeros((U, 4), dtype=torch.int64, device="cuda")
    itc = torch.zeros((U, 2), dtype=torch.int64, device="cuda")
    for n in (1, 2):
        ldpc.count(dev(hard.reshape(-1, N)), dev(skip.reshape(-1)), B, U, C, K, counts, dev(iters.reshape(-1)), itc)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), n * want) and np.array_equal(itc.cpu().numpy(), n * want_it)
    plain = torch.zeros((U, 4), dtype=torch.int64, device="cuda")
    ldpc.count(dev(hard.reshape(-1, N)), dev(skip.reshape(-1)), B, U, C, K, plain)
    torch.cuda.synchronize()
    assert np.array_equal(plain.cpu().numpy(), want)


# ------------------------------------------------------------------ E1: end to end
EB, EBNO = 64, (0.0, 12.0)
EKW = dict(max_mc_iter=1, num_target_block_errors=10 ** 9, early_stop=False)


@functools.lru_cache(maxsize=None)
def _setup():
    from neural_rx_amd import weights as W
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator
    from neural_rx_amd.receiver import CGNNEngine, spec_for
    cfg = get_config("nrx_rt")
    engine = CGNNEngine(spec_for(cfg), W.load(cfg.label))
    p = GenParams.from_config(cfg, num_prbs=4)
    return cfg, engine, p, SlotGenerator(p, want_h=True)


@functools.lru_cache(maxsize=None)
def _sim(system, with_coded):
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.evaluate import sim_ber, sim_ber_baseline
    cfg, engine, p, gen = _setup()
    points = [] if with_coded else None
    if system == "nrx":
        res = sim_ber(engine, gen, EBNO, EB, num_it=cfg.num_nrx_iter_eval, coded=points, **EKW)
    else:
        res = sim_ber_baseline(BaselineReceiver(system, p), gen, EBNO, EB, coded=points, **EKW)
    return res, points


def _oracle_chain(system):
    """per Eb/N0 point the coded counters of the numpy chain on the receiver's own LLRs of the loop's slots"""
    import torch
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.generator import ebno_to_no
    from neural_rx_amd.receiver import compute_pe
    cfg, engine, p, gen = _setup()
    pe = torch.from_numpy(compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)).cuda()
    rx = None if system == "nrx" else BaselineReceiver(system, p)
    code, C = ldpc.fit("r12", p.num_subcarriers * (14 - len(p.dmrs_symbols)) * max(p.mcs_bits))
    out = []
    for k, ebno in enumerate(EBNO):
        no = ebno_to_no(ebno, len(p.dmrs_symbols))
        sb = gen(EB, no, slot_offset=k * EB)
        if rx is None:
            llr, _ = engine.forward(sb.y, pe, sb.h_hat, sb.active, num_it=cfg.num_nrx_iter_eval)
        else:
            llr = rx(sb, no)
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()  # noqa: E731
        llr_in, skip = R.gather(host(llr), host(sb.bits), host(sb.mcs), host(sb.active), p.mcs_bits, p.dmrs_symbols,
                                C, code.n, code.n)
        dec = R.decode(code, llr_in, 20, early_stop=True, skip=skip)
        out.append(R.count(dec["hard"], skip, EB, p.num_tx, C, code.num_info, dec["iters"]))
    return code, C, out


@pytest.mark.parametrize("system", ["baseline_perf_csi_lmmse", "nrx"])
def test_e1_coded_evaluation(system):
    """E1: nrx_rt, 4 PRB, 2 users, B = 64, r12 (N = 2304, one codeword per (slot, user)), Eb/N0 0 and 12 dB.
    The coded counters equal the oracle chain on the same LLRs with at most 2 blocks different per point;
    the coded BLER falls from the low to the high point; the uncoded SimResult is the one of a run
    without ``coded``."""
    plain, none = _sim(system, False)
    res, points = _sim(system, True)
    assert none is None and len(points) == len(EBNO)
    assert res.counts == plain.counts and res.ber == plain.ber and res.bler == plain.bler
    assert res.mc_iters == plain.mc_iters and res.slots == plain.slots and res.ebno_db == plain.ebno_db
    code, C, chain = _oracle_chain(system)
    assert (code.n, code.z, C) == (2304, 96, 1)
    for ebno, cr, (want, want_it) in zip(EBNO, points, chain):
        w = want.sum(0)
        print(f"{system} {ebno:5.1f} dB: coded BER {cr.ber:.3e} BLER {cr.bler:.3e} iterations {cr.mean_iters:.2f}  "
              f"counts {cr.counts}  oracle {w.tolist()} iterations {want_it.sum(0).tolist()}")
        assert (cr.code, cr.rate, cr.n, cr.z, cr.cw_per_block) == ("r12", 0.5, 2304, 96, 1)
        assert cr.counts[1] == w[1] == EB * 2 * 1152 and cr.counts[3] == w[3] == EB * 2
        assert cr.codewords == want_it.sum(0)[1] == EB * 2
        assert abs(cr.counts[2] - w[2]) <= 2
    assert points[1].bler < points[0].bler
