"""numpy float64 statement of the cover-coded DMRS ports of ``nrx_generate_slots_dmrs`` and of the
despreading LS estimator ``nrx_ls_estimate`` (include/nrx.h).  A test helper, not a test.

Ports.  Port u is (g, wf, wt): the comb offset (CDM group), a frequency cover and a time cover.  This
project's rule for the default assignment -- the arrangement of DMRS configuration type 1 -- is

    g = (u >> 1) & 1,   wf = u & 1,   wt = (u >> 2) & 1          (``default_ports``)

so ports 0 and 2 are the two uncovered ports of the two groups.

Base sequence.  r[g][j][k] = s0 + j s1 with s = 1 - 2 bit, bits 0 and 1 of word 0 of the Philox draw
(seed, slot 0, stream 7, element (g Pmax + j) 4 + k), j = f >> 1 the position on the comb, k the position
in ``dmrs_symbols``, Pmax = (F + 1) // 2: amplitude sqrt(2), both parts exact in f32, a function of the
seed alone.

Pilots.  x_u[f, t_k] = active r[g][j][k] (-1)^(wf (j & 1)) (-1)^(wt (k & 1)) on f mod 2 = g, 0 elsewhere.

Estimator.  With z[j, k, a] = y[f, t_k, a] conj(p) / |p|^2, p = pilots[g][j][k]:

    h_ls_u[j, k, a] = mean over j' in {j, j ^ 1 if despread_f}, k' in {k, k ^ 1 if despread_t} of
                      (-1)^(wf (j' & 1) + wt (k' & 1)) z[j', k', a]

``h_hat`` is h_ls at the port's nearest own pilot (``oracle.synth_ref.nearest_pilot``); the Aerial list
holds (-1)^(wf (j & 1)) times the mean over the time pair only, at p = k F / 2 + j.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S

STREAM_DMRS = 7


def default_ports(num_tx: int):
    """(cdm_group, focc, tocc), each a list of num_tx entries"""
    u = np.arange(num_tx)
    return list((u >> 1) & 1), list(u & 1), list((u >> 2) & 1)


def base_sequence(seed: int, num_subcarriers: int, num_dmrs_symbols: int) -> np.ndarray:
    """r [2, Pmax, nd] complex128"""
    pmax = (num_subcarriers + 1) // 2
    g, j, k = np.meshgrid(np.arange(2), np.arange(pmax), np.arange(num_dmrs_symbols), indexing="ij")
    w0 = S.draw(seed, 0, STREAM_DMRS, (g * pmax + j) * 4 + k)[0]
    one = np.uint64(1)
    return (1.0 - 2.0 * (w0 & one).astype(np.float64)) + 1j * (1.0 - 2.0 * ((w0 >> one) & one).astype(np.float64))


def pilot_table(r: np.ndarray) -> np.ndarray:
    """[2, Pmax, nd, 2] float32, the layout of nrx_ls_io.pilots"""
    return np.stack([r.real, r.imag], -1).astype(np.float32)


def cover(wf: int, wt: int, nj: int, nk: int) -> np.ndarray:
    """(-1)^(wf (j & 1) + wt (k & 1)), [nj, nk]"""
    j, k = np.arange(nj)[:, None], np.arange(nk)[None, :]
    return 1.0 - 2.0 * ((wf * (j & 1) + wt * (k & 1)) & 1)


def port_pilots(r: np.ndarray, ports, num_subcarriers: int, dmrs_symbols: Sequence[int], num_symbols: int = 14):
    """x [U, F, T] complex128: the pilots of every port (active = 1), zeros off its comb and off the DMRS symbols"""
    grp, focc, tocc = ports
    F, nd = num_subcarriers, len(dmrs_symbols)
    x = np.zeros((len(grp), F, num_symbols), np.complex128)
    for u, (g, wf, wt) in enumerate(zip(grp, focc, tocc)):
        f = np.arange(g, F, 2)
        c = cover(wf, wt, r.shape[1], nd)[f >> 1]
        x[u][np.ix_(f, list(dmrs_symbols))] = r[g][f >> 1] * c
    return x


def ls_estimate(y: np.ndarray, pilots: np.ndarray, dmrs_symbols: Sequence[int], ports, despread_f: bool,
                despread_t: bool, active: Optional[np.ndarray] = None):
    """y [B, F, T, 2A] f32, pilots [2, Pmax, nd, 2] f32 -> (h_ls, h_pair), complex128 [B, U, Pmax, nd, A]:
    the estimate, and the estimate before frequency despreading (the Aerial list's values).  Comb positions
    outside the grid (2 j + g >= F) hold zeros."""
    grp, focc, tocc = ports
    B, F, T, A2 = y.shape
    A, nd, U = A2 // 2, len(dmrs_symbols), len(grp)
    pmax = (F + 1) // 2
    yc = y[..., :A].astype(np.float64) + 1j * y[..., A:].astype(np.float64)
    p = pilots[..., 0].astype(np.float64) + 1j * pilots[..., 1].astype(np.float64)
    h_ls = np.zeros((B, U, pmax, nd, A), np.complex128)
    h_pair = np.zeros_like(h_ls)
    jj, kk = np.arange(pmax), np.arange(nd)
    for u, (g, wf, wt) in enumerate(zip(grp, focc, tocc)):
        f = np.arange(g, F, 2)
        n = len(f)
        z = yc[:, f][:, :, list(dmrs_symbols)] * (np.conj(p[g, :n]) / np.abs(p[g, :n]) ** 2)[None, :, :, None]
        z = z * cover(wf, wt, n, nd)[None, :, :, None]
        zt = (z + z[:, :, kk ^ 1]) / 2 if despread_t else z
        zf = (zt + zt[:, jj[:n] ^ 1]) / 2 if despread_f else zt
        on = np.ones(B) if active is None else (active[:, u] > 0)
        h_ls[:, u, :n] = zf * on[:, None, None, None]
        # the own cover of the frequency pair stays on it: z above is already multiplied by it
        h_pair[:, u, :n] = zt * on[:, None, None, None]
    return h_ls, h_pair


def h_hat(h_ls: np.ndarray, ports, num_subcarriers: int, dmrs_symbols: Sequence[int], num_symbols: int = 14):
    """[B, U, F, T, 2A] f32: h_ls at the nearest own pilot (zeros where the port has no pilot in the grid)"""
    grp = ports[0]
    B, U, _, nd, A = h_ls.shape
    F, T = num_subcarriers, num_symbols
    kof = {t: k for k, t in enumerate(dmrs_symbols)}
    out = np.zeros((B, U, F, T, A), np.complex128)
    for u in range(U):
        if grp[u] >= F:
            continue
        fp, tp = S.nearest_pilot(F, dmrs_symbols, grp[u], T)
        kp = np.vectorize(kof.get)(tp)
        out[:, u] = h_ls[:, u, fp >> 1, kp]
    return np.concatenate([out.real, out.imag], -1).astype(np.float32)


def aerial_list(h_pair: np.ndarray, num_subcarriers: int):
    """(h_ls_real, h_ls_imag) [B, Npil, U, A] f32, p = k F / 2 + j (needs F % 12 == 0)"""
    B, U, pmax, nd, A = h_pair.shape
    assert num_subcarriers % 12 == 0 and pmax == num_subcarriers // 2
    v = h_pair.transpose(0, 3, 2, 1, 4).reshape(B, nd * pmax, U, A)
    return v.real.astype(np.float32), v.imag.astype(np.float32)


def generate(spec: S.GenSpec, ports):
    """The generator with cover-coded ports on top of ``oracle.synth_ref.generate`` (whose cdm_group must
    be ports[0]): (GenOut of the uncovered run, y [B, F, T, 2A] f32, x' [B, U, F, T], r).  Only the pilot REs
    move:  y' = y_c + sum_u h_u (x'_u - x_u), with h the f32 ``GenOut.h``, whose rounding contributes at most
    2^-25 |h_u| |x'_u - x_u| <= 2^-25 2 sqrt(2) |h_u| per port to y'."""
    assert list(spec.cdm_group[:spec.num_tx]) == [int(g) for g in ports[0]]
    g = S.generate(spec)
    A, T = spec.num_rx_ant, spec.num_symbols
    r = base_sequence(spec.seed, spec.num_subcarriers, len(spec.dmrs_symbols))
    xp = port_pilots(r, ports, spec.num_subcarriers, spec.dmrs_symbols, T)[None] * g.active[:, :, None, None]
    dm = np.zeros(T, bool)
    dm[list(spec.dmrs_symbols)] = True
    x2 = np.where(dm[None, None, None, :], xp, g.x)
    h = g.h[..., :A].astype(np.float64) + 1j * g.h[..., A:].astype(np.float64)          # [B, U, F, T, A]
    y_c = g.y_c + np.einsum("bufta,buft->baft", h, x2 - g.x)
    y = np.moveaxis(y_c, 1, -1)
    return g, np.concatenate([y.real, y.imag], -1).astype(np.float32), x2, r
