"""The numpy statement of the cover-coded DMRS ports and the despreading LS estimator
(tests/dmrs_ref.py), the port rule of ``neural_rx_amd/ls.py``, and the filter design for despread
pilots (``chest.lmmse_design(despread_f=True)``) against the brute-force Kronecker solve; no GPU."""
import numpy as np
import pytest

from neural_rx_amd.generator import GenParams
from neural_rx_amd.ls import DMRSPorts

from tests import chest_ref as R
from tests import dmrs_ref as D

NO = 0.23


def test_port_rule():
    p = DMRSPorts.default(8)
    assert (list(p.cdm_group), list(p.focc), list(p.tocc)) == tuple(map(list, D.default_ports(8)))
    assert p.cdm_group == (0, 0, 1, 1, 0, 0, 1, 1) and p.focc == (0, 1) * 4 and p.tocc == (0,) * 4 + (1,) * 4
    assert p.despread_f and p.despread_t and p.block == 4
    q = DMRSPorts.from_ports([0, 2])            # the two-user configs: groups 0 / 1, no cover in use
    assert q.cdm_group == (0, 1) and not q.despread_f and not q.despread_t and q.block == 1
    assert DMRSPorts.default(4).block == 2 and not DMRSPorts.default(4).despread_t
    with pytest.raises(ValueError):
        DMRSPorts([0, 0], [1, 1], [0, 0])       # the same port twice
    with pytest.raises(ValueError):
        DMRSPorts.default(9)
    with pytest.raises(ValueError):
        DMRSPorts.default(4).validate(22, (2, 11))
    with pytest.raises(ValueError):
        DMRSPorts.default(8).validate(24, (2, 11))
    with pytest.raises(ValueError):
        DMRSPorts.default(8).validate(24, (2, 3, 10))
    DMRSPorts.default(8).validate(24, (2, 3, 10, 11))
    DMRSPorts.from_ports([0, 2]).validate(13, (2, 7, 11))


def test_the_eight_covers_are_orthogonal_over_a_block():
    grp, focc, tocc = D.default_ports(8)
    v = np.zeros((8, 2, 2, 2))                  # [port][comb offset][j][k]
    for u in range(8):
        v[u, grp[u]] = D.cover(focc[u], tocc[u], 2, 2)
    g = np.einsum("ugjk,vgjk->uv", v, v)
    assert np.array_equal(g, 4 * np.eye(8))


def test_base_sequence_is_a_function_of_the_seed():
    r = D.base_sequence(1234, 24, 4)
    assert r.shape == (2, 12, 4) and np.all(np.abs(r.real) == 1) and np.all(np.abs(r.imag) == 1)
    assert np.array_equal(r[:, :, :2], D.base_sequence(1234, 24, 2))         # element index (g Pmax + j) 4 + k
    assert not np.array_equal(r, D.base_sequence(1235, 24, 4))
    assert 0.2 < np.mean(r.real > 0) < 0.8 and 0.2 < np.mean(r.imag > 0) < 0.8
    t = D.pilot_table(r)
    assert t.dtype == np.float32 and t.shape == (2, 12, 4, 2) and np.array_equal(t[..., 0] + 1j * t[..., 1], r)


def _block_constant_case(F=24, A=3, dmrs=(2, 3, 10, 11), seed=5):
    """8 active ports, a channel constant over every 2 x 2 pilot block with entries on a 1/8 grid, so that
    y is exact in float32"""
    rng = np.random.default_rng(seed)
    ports = D.default_ports(8)
    r = D.base_sequence(seed, F, len(dmrs))
    x = D.port_pilots(r, ports, F, dmrs)                                     # [U, F, T]
    hb = (rng.integers(-8, 9, (8, F // 4, 2, A)) + 1j * rng.integers(-8, 9, (8, F // 4, 2, A))) / 8.0
    h = np.zeros((8, F, 14, A), complex)
    for i, t in enumerate(dmrs):
        h[:, :, t] = np.repeat(hb[:, :, i // 2], 4, axis=1)
    yc = np.einsum("ufta,uft->fta", h, x)[None]
    y = np.concatenate([yc.real, yc.imag], -1).astype(np.float32)
    assert np.array_equal(y[..., :A] + 1j * y[..., A:].astype(np.float64), yc)
    return ports, r, x, h, y, dmrs


def test_despreading_returns_every_ports_channel_on_a_block_constant_channel():
    ports, r, x, h, y, dmrs = _block_constant_case()
    h_ls, _ = D.ls_estimate(y, D.pilot_table(r), dmrs, ports, True, True)
    for u in range(8):
        f = np.arange(ports[0][u], 24, 2)
        want = h[u][f][:, list(dmrs)]                                        # [j, k, A]
        assert np.abs(h_ls[0, u] - want).max() <= 1e-12
    hh = D.h_hat(h_ls, ports, 24, dmrs)
    hc = hh[0, ..., :3] + 1j * hh[0, ..., 3:]
    for u in range(8):                                                       # h_hat at the own pilots is h_ls there
        f = np.arange(ports[0][u], 24, 2)
        assert np.abs(hc[u][f][:, list(dmrs)] - h[u][f][:, list(dmrs)]).max() <= 1e-6
    # without despreading the ports of a group collide
    raw, _ = D.ls_estimate(y, D.pilot_table(r), dmrs, ports, False, False)
    assert np.abs(raw[0, 0] - h[0][0::2][:, list(dmrs)]).max() > 0.1


def test_despreading_is_ls_with_the_own_covered_pilot_then_the_pair_average():
    """the Aerial formulation: y / x_u at the own pilots, then the mean over the block"""
    rng = np.random.default_rng(7)
    F, A, dmrs = 24, 2, (2, 3, 10, 11)
    ports = D.default_ports(8)
    r = D.base_sequence(9, F, 4)
    x = D.port_pilots(r, ports, F, dmrs)
    y = rng.standard_normal((2, F, 14, 2 * A)).astype(np.float32)
    yc = y[..., :A].astype(np.float64) + 1j * y[..., A:]
    h_ls, h_pair = D.ls_estimate(y, D.pilot_table(r), dmrs, ports, True, True)
    for u in range(8):
        f = np.arange(ports[0][u], F, 2)
        ls = yc[:, f][:, :, list(dmrs)] / x[u][f][:, list(dmrs)][None, :, :, None]          # [B, j, k, A]
        tp = (ls[:, :, 0::2] + ls[:, :, 1::2]) / 2
        assert np.abs(h_pair[:, u] - np.repeat(tp, 2, axis=2)).max() <= 1e-12
        blk = (tp[:, 0::2] + tp[:, 1::2]) / 2
        assert np.abs(h_ls[:, u] - np.repeat(np.repeat(blk, 2, axis=1), 2, axis=2)).max() <= 1e-12
    re, im = D.aerial_list(h_pair, F)
    assert re.shape == (2, 4 * 12, 8, A)
    # the pair average of the Aerial front end (p, p ^ 1) is the frequency despreading
    v = re.astype(np.float64) + 1j * im
    pair = (v + v[:, np.arange(48) ^ 1]) / 2
    want = h_ls.transpose(0, 3, 2, 1, 4).reshape(2, 48, 8, A)
    assert np.abs(pair - want).max() <= 1e-6


def test_inactive_ports_and_plain_ls():
    rng = np.random.default_rng(3)
    F, A, dmrs = 13, 2, (2, 7, 11)
    ports = ([0, 1], [0, 0], [0, 0])
    p = rng.standard_normal((2, 7, 3, 2)).astype(np.float32) + 2.0           # any non-zero values
    y = rng.standard_normal((3, F, 14, 2 * A)).astype(np.float32)
    act = np.array([[1, 1], [0, 1], [1, 0]], np.float32)
    h_ls, h_pair = D.ls_estimate(y, p, dmrs, ports, False, False, act)
    assert np.array_equal(h_ls, h_pair)
    assert np.all(h_ls[1, 0] == 0) and np.all(h_ls[2, 1] == 0) and np.all(h_ls[0, 1, 6] == 0)   # group 1: 6 pilots
    pc = p[..., 0].astype(np.float64) + 1j * p[..., 1]
    want = (y[0, 3, 7, :A] + 1j * y[0, 3, 7, A:].astype(np.float64)) / pc[1, 1, 1]
    assert np.abs(h_ls[0, 1, 1, 1] - want).max() <= 1e-12
    hh = D.h_hat(h_ls, ports, F, dmrs)
    assert np.allclose(hh[0, 1, 0, 0, :A], h_ls[0, 1, 0, 0].real.astype(np.float32))    # f = 0 -> pilot 1, t = 0 -> symbol 2
    assert np.allclose(hh[0, 1, 4, 9, A:], h_ls[0, 1, 1, 1].imag.astype(np.float32))    # f = 4 -> 3, t = 9: 7 and 11 tie, first wins


@pytest.mark.parametrize("F", [12, 24])
def test_despread_design_equals_the_kronecker_solve(F):
    """chest.lmmse_design(despread_f=True) is the brute-force 2-D Wiener filter of the despread
    observations o_q = (h[P_2q] + h[P_2q+1]) / 2 with noise variance sigma^2 / 2, and its error map
    the brute-force one, to 1e-10 (the gate of tests/test_chest_ref.py), nd = 2"""
    from neural_rx_amd.chest import lmmse_design
    dmrs, T = (2, 11), 14
    R_f, R_t = R.model_covariance(F)
    R_f, R_t = 1.1 * R_f, 0.9 * R_t
    p = GenParams(num_tx=2, num_subcarriers=F, num_rx_ant=2, dmrs_symbols=dmrs)
    d = lmmse_design(R_f, R_t, p, NO, dtype=np.float64, despread_f=True)
    plain = lmmse_design(R_f, R_t, p, NO, dtype=np.float64)
    cx = lambda a: a[..., 0] + 1j * a[..., 1]  # noqa: E731
    W, a, v = cx(d.filt), cx(d.tcoef), cx(d.vconj)
    Rt = R_t / R_t[0, 0].real
    for g in (0, 1):
        P = R.pilots(F, g)
        S = np.kron(np.eye(len(P) // 2), [[0.5, 0.5]])
        C = np.kron(Rt[:, dmrs], R_f[:, P] @ S.T)                                        # rows (t, f), columns (d, q)
        Coo = np.kron(Rt[np.ix_(dmrs, dmrs)], S @ R_f[np.ix_(P, P)] @ S.T)
        Wb = C @ np.linalg.inv(Coo + (NO / 4.0) * np.eye(Coo.shape[0]))
        err = (R_f[0, 0].real - np.real(np.sum(Wb * np.conj(C), axis=1))).reshape(T, F).T
        Wb = Wb.reshape(T, F, 2, len(P) // 2).transpose(1, 0, 2, 3)                      # [F, T, nd, Q]
        full = np.einsum("kt,kd,kfp->ftdp", a, v, W[g][:, :, :len(P)])                   # on the pilots as they lie
        assert np.array_equal(full[..., 0::2], full[..., 1::2])                          # both pilots of a pair: W' / 2
        assert np.abs(2 * full[..., 0::2] - Wb).max() <= 1e-10
        assert np.abs(d.err_var[g] - err).max() <= 1e-10
        assert err.min() > 0 and err.max() < R_f[0, 0].real
        assert np.abs(d.err_var[g] - plain.err_var[g]).max() > 1e-6                      # not the undespread design
    with pytest.raises(ValueError):
        lmmse_design(R_f[:10, :10], R_t, GenParams(num_tx=2, num_subcarriers=10, num_rx_ant=2), NO, despread_f=True)


def test_receivers_under_cover(monkeypatch):
    """err_var over the despreading block, no contamination note, and the refused combinations"""
    from neural_rx_amd import _lib, baseline, cfo, chest
    monkeypatch.setattr(_lib, "load", lambda *a, **k: None)      # no launch here: the library is not needed
    p4 = GenParams(num_tx=4, num_subcarriers=24, num_rx_ant=4, dmrs=DMRSPorts.default(4))
    p8 = GenParams(num_tx=8, num_subcarriers=24, num_rx_ant=4, dmrs_symbols=(2, 3, 10, 11), dmrs=DMRSPorts.default(8))
    plain = GenParams(num_tx=4, num_subcarriers=24, num_rx_ant=4, cdm_group=(0, 1, 0, 1))
    assert p4.cdm_group == (0, 0, 1, 1)
    for p, n in ((p4, 2), (p8, 4)):
        rx = baseline.BaselineReceiver("baseline_lsnn_lmmse", p)
        assert rx.err_var(0.5) == p.num_tx * 0.5 / (2 * n) and not rx.contaminated
    rx = baseline.BaselineReceiver("baseline_lsnn_lmmse", plain)
    assert rx.err_var(0.5) == 4 * 0.5 / 2 and rx.contaminated
    lin = chest.EstimatorBaselineReceiver("baseline_lslin_lmmse", p4)
    assert lin.err_var(0.5) == 4 * 0.5 / 4 and not lin.contaminated
    R_f, R_t = R.model_covariance(24)
    lm = chest.EstimatorBaselineReceiver("baseline_lmmse_lmmse", p4, R_f=R_f, R_t=R_t)
    un = chest.EstimatorBaselineReceiver("baseline_lmmse_lmmse", plain, R_f=R_f, R_t=R_t)
    assert 0 < lm.err_var(0.5) and lm.err_var(0.5) != un.err_var(0.5)
    with pytest.raises(ValueError, match="3-D"):
        chest.ChannelEstimator("lmmse3", p4)
    for kind in chest.KINDS:
        with pytest.raises(ValueError, match="time"):
            chest.ChannelEstimator(kind, p8)
    with pytest.raises(ValueError, match="time"):
        cfo.CFOCompensator(p8)
    cfo.CFOCompensator(p4)
    with pytest.raises(ValueError):
        GenParams(num_tx=4, num_subcarriers=22, num_rx_ant=4, dmrs=DMRSPorts.default(4))
    with pytest.raises(ValueError):
        GenParams(num_tx=3, num_subcarriers=24, num_rx_ant=4, dmrs=DMRSPorts.default(4))
