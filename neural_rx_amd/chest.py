"""Channel-estimation baselines on the GPU: covariance estimation, 2-D LMMSE and linear interpolation.

The counterpart of the estimators of the reference's ``BaselineReceiver`` (utils/baseline_rx.py:
100-229) for ``baseline_lmmse_lmmse`` and ``baseline_lslin_lmmse``, and of its
``scripts/compute_cov_mat.py`` (which ``scripts/evaluate.py:159`` runs before every baseline
evaluation).  The device work is in ``libnrx.so`` (``nrx_cov_accumulate``, ``nrx_cov_space_accumulate``,
``nrx_chest_lmmse``, ``nrx_chest_lmmse3``, ``nrx_chest_lin``: include/nrx.h, csrc/nrx_chest.hip); torch tensors are only device containers and
a missing library is an error, never a host fallback.  The filter design is host numpy float64, run
once per noise level: it is not hot.

Three stated departures from the reference (Sionna):

* **Toeplitz covariance.**  ``CovarianceEstimator`` estimates lags, not full matrices: the
  generator's channel is stationary in frequency and time by construction (oracle/synth_ref.py:
  206-226), so ``R_f`` and ``R_t`` are Hermitian Toeplitz and the lags estimate the same quantity
  with less variance and O(F) storage.  On the default channel the spatial covariance is the
  identity -- the taps are drawn i.i.d. per antenna (synth_ref.py:213-217) -- so the ``s`` stage of
  the reference's order ``"s-f-t"`` is a no-op there and ``"lmmse"`` leaves it out.  With
  receive-antenna correlation (``GenParams.rx_corr``, ``generator.scenario``) it is not:
  ``CovarianceEstimator.space()`` estimates ``R_s`` and ``"lmmse3"`` (``lmmse3_design``,
  ``nrx_chest_lmmse3``) is the exact filter under ``R_s (x) R_t (x) R_f``, the counterpart of the
  covariance the reference hands to its estimator (utils/baseline_rx.py:160-195).  As in the
  reference there is one ``R_f``, ``R_t``, ``R_s`` for all users -- with per-user profiles, the
  mixture over them; per-user covariances are out of scope.
* **Exact 2-D filter.**  Sionna's ``LMMSEInterpolator`` filters sequentially ("f-t"), which
  approximates the 2-D Wiener filter.  Here the estimate is the exact filter under the separable
  covariance ``R_t (x) R_f``, in an eigen form of ``R_t[D, D]`` that costs ``nd`` frequency GEMMs
  (``lmmse_design``), on the full band up to 3300 subcarriers (the reference splits grids above
  100 PRB into blocks).  The baseline is therefore, if anything, stronger than the reference's.
* **Scalar err_var.**  Sionna hands the detector a per-RE error variance; ``nrx_lmmse_detect`` takes
  one scalar.  ``EstimatorBaselineReceiver`` passes ``num_active x`` the mean of the theoretical
  error map over the data symbols (lmmse), or ``num_active * no / 2`` as ``baseline_lsnn_lmmse``
  does (lin).  Both are approximations of the per-RE quantity.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib
from ._call import Workspace, fill_dmrs, fill_grid, ptr, ref, require, stream_of, torch as _torch
from .baseline import Receiver
from .generator import NUM_SYMBOLS, GenParams, SlotBatch

SYSTEMS = ("baseline_lslin_lmmse", "baseline_lmmse_lmmse")
KINDS = ("lin", "lmmse", "lmmse3")
COV_SLOT_OFFSET = 1 << 40        # covariance slots start here: disjoint from every Monte-Carlo offset


def toeplitz(lags: np.ndarray) -> np.ndarray:
    """Hermitian Toeplitz R[i, j] = lags[i - j] (i >= j), conj(lags[j - i]) (i < j)."""
    lags = np.asarray(lags, np.complex128)
    n = len(lags)
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    return np.where(d >= 0, lags[np.abs(d)], np.conj(lags[np.abs(d)]))


def pilot_subcarriers(num_subcarriers: int, group: int) -> np.ndarray:
    return np.arange(group, num_subcarriers, 2)


class CovarianceEstimator:
    """Frequency and time covariance of the generator's channel from its true ``h``
    (``SlotGenerator(want_h=True)``): ``accumulate(sb)`` adds a batch's lag sums on the device
    (``nrx_cov_accumulate``, float64, deterministic), ``matrices()`` divides by the product counts
    and returns the Hermitian Toeplitz ``(R_f [F, F], R_t [14, 14])`` as numpy complex128.
    ``accumulate`` also adds the spatial sums (``nrx_cov_space_accumulate``); ``space()`` returns
    ``R_s [A, A]``, the identity up to estimation noise unless the generator correlates its
    antennas (module docstring).  ``accumulate(..., workspace=(ws, ws_space))`` runs the two launches
    in the caller's uint8 device tensors (any content) instead of the estimator's own;
    ``last_workspace_bytes`` is the pair of sizes the ``*_workspace_size`` calls asked for."""

    def __init__(self, params: GenParams, device: int = 0):
        torch = _torch()
        self.p = params
        self.device = device
        self._lib = _lib.load()
        self.acc = torch.zeros((params.num_subcarriers + NUM_SYMBOLS, 2), dtype=torch.float64,
                               device=f"cuda:{device}")
        self.acc_s = torch.zeros((params.num_rx_ant, params.num_rx_ant, 2), dtype=torch.float64,
                                 device=f"cuda:{device}")
        self.slots = 0
        self._ws = (Workspace(), Workspace())
        self.last_workspace_bytes = (0, 0)

    def accumulate(self, sb: SlotBatch, stream=None, workspace=None) -> None:
        h = sb.h
        if h is None:
            raise ValueError("the covariance needs the true channel: SlotGenerator(want_h=True)")
        p, lib, dev = self.p, self._lib, self.acc.device
        B = h.shape[0]
        require("h", h, (B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, 2 * p.num_rx_ant), _torch().float32, dev)

        def plan(ws, cls, acc, size_fn, given):
            """(descriptor, bytes asked, buffer) of one of the two launches: their descriptors are field for
            field the same"""
            d = cls()
            fill_grid(d, B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, p.num_rx_ant)
            d.h, d.acc = h.data_ptr(), acc.data_ptr()
            n = ws.size(size_fn, ref(d))
            return d, n, ws.get(n, dev, given)

        given = workspace if workspace is not None else (None, None)
        lag = plan(self._ws[0], _lib.nrx_cov_io, self.acc, lib.nrx_cov_workspace_size, given[0])
        spc = plan(self._ws[1], _lib.nrx_cov_space_io, self.acc_s, lib.nrx_cov_space_workspace_size, given[1])
        self.last_workspace_bytes = (lag[1], spc[1])
        stream = stream_of(dev, stream)
        for (d, _, ws), run in ((lag, lib.nrx_cov_accumulate), (spc, lib.nrx_cov_space_accumulate)):
            _lib.check(run(ref(d), ws.data_ptr(), ws.numel(), stream))
        self.slots += B

    def lags(self):
        """(r_f [F], r_t [14]) complex128: the lag sums over their product counts"""
        if not self.slots:
            raise ValueError("no slots accumulated")
        p = self.p
        F, T = p.num_subcarriers, NUM_SYMBOLS
        a = self.acc.cpu().numpy()
        s = a[:, 0] + 1j * a[:, 1]
        n = self.slots * p.num_tx * p.num_rx_ant
        return s[:F] / (n * T * (F - np.arange(F))), s[F:] / (n * F * (T - np.arange(T)))

    def matrices(self):
        r_f, r_t = self.lags()
        return toeplitz(r_f), toeplitz(r_t)

    def space(self) -> np.ndarray:
        """``R_s [A, A]`` complex128, scaled to ``trace = A`` and made exactly Hermitian: the
        spatial covariance ``E h[a] conj(h[a'])`` over every (slot, user, RE).  One matrix for all
        users, as ``R_f`` and ``R_t`` are -- the mixture over the users' profiles, which is what
        the reference's compute_cov_mat.py estimates."""
        if not self.slots:
            raise ValueError("no slots accumulated")
        a = self.acc_s.cpu().numpy()
        R = a[..., 0] + 1j * a[..., 1]
        R = 0.5 * (R + R.conj().T)
        return R * (self.p.num_rx_ant / np.trace(R).real)


@dataclasses.dataclass
class LMMSEDesign:
    """Tables of ``nrx_chest_lmmse`` (include/nrx.h) and the theoretical error variance."""
    filt: np.ndarray        # [2, nd, F, Pmax, 2] f32: W_k of CDM group 0 / 1 (re, im)
    tcoef: np.ndarray       # [nd, 14, 2] f32: a_k[t]
    vconj: np.ndarray       # [nd, nd, 2] f32: conj(v_k[d])
    err_var: np.ndarray     # [2, F, 14] f64: E |h - h^|^2 per RE of a user of CDM group 0 / 1
    no: float


def lmmse_design(R_f: np.ndarray, R_t: np.ndarray, params: GenParams, no: float, dtype=np.float32,
                 despread_f: bool = False) -> LMMSEDesign:
    """The exact 2-D Wiener filter under ``R_t (x) R_f`` for LS estimates at the own pilots
    ``P = {f : f mod 2 = group}`` of the DMRS symbols ``D`` with noise ``sigma^2 = no / 2`` (the
    generator's pilots have energy 2), in the eigen form of ``R_t[D, D] = V diag(lambda) V^H``:

        W_k = R_f[:, P] (R_f[P, P] + (sigma^2 / lambda_k) I)^-1,    a_k[t] = R_t[t, D] v_k / lambda_k
        h^[f, t] = sum_k a_k[t] (W_k z_k)[f],                       z_k = sum_d conj(v_k[d]) h_ls[P, D_d]

    which equals ``(R_t[:, D] (x) R_f[:, P]) (R_t[D, D] (x) R_f[P, P] + sigma^2 I)^-1`` (checked
    against that brute-force form in tests/test_chest_ref.py).  ``R_t`` is scaled to a unit diagonal
    first, so the prior variance of an RE is ``R_f[0, 0]`` (both matrices estimate the same power).
    The error map is ``e[f, t] = R_f[0, 0] - sum_j W_ij conj(C_ij)`` with ``C = R_t[:, D] (x) R_f[:, P]``,
    from the unrounded filter.  Components with ``lambda_k <= 1e-12 lambda_max`` are dropped (zero
    tables).  The tables are rounded once to float32, the kernel's format (``dtype=np.float64``
    keeps them unrounded, for checks).

    ``despread_f``: the pilots hold frequency-despread LS estimates (``ls.py``, cover-coded ports): both
    pilots of a pair (P_2q, P_2q+1) hold ``o_q = (h[P_2q] + h[P_2q+1]) / 2`` plus noise of variance
    ``sigma^2 / 2``.  With ``S`` the |P|/2 x |P| averaging matrix the filter of the observations is

        W'_k = R_f[:, P] S^T (S R_f[P, P] S^T + (sigma^2 / (2 lambda_k)) I)^-1

    and the kernel's table, which multiplies the pilots as they lie in ``h_hat``, is
    ``W[:, 2q] = W[:, 2q+1] = W'[:, q] / 2``; the error map follows from ``W'``.  Needs F % 4 == 0."""
    if not no > 0:
        raise ValueError("no must be > 0")
    if despread_f and params.num_subcarriers % 4:
        raise ValueError("despread_f needs num_subcarriers % 4 == 0")
    F, T = params.num_subcarriers, NUM_SYMBOLS
    D = list(params.dmrs_symbols)
    nd = len(D)
    R_f = np.asarray(R_f, np.complex128)
    R_t = np.asarray(R_t, np.complex128)
    if R_f.shape != (F, F) or R_t.shape != (T, T):
        raise ValueError(f"R_f must be {(F, F)} and R_t {(T, T)}")
    R_t = R_t / R_t[0, 0].real
    sigma2 = float(no) / 2.0
    lam, V = np.linalg.eigh(R_t[np.ix_(D, D)])
    Pmax = (F + 1) // 2
    filt = np.zeros((2, nd, F, Pmax), np.complex128)
    tcoef = np.zeros((nd, T), np.complex128)
    vconj = np.zeros((nd, nd), np.complex128)
    err = np.full((2, F, T), R_f[0, 0].real)
    for k in range(nd):
        if lam[k] <= 1e-12 * lam[-1]:
            continue
        v = V[:, k]
        tcoef[k] = (R_t[:, D] @ v) / lam[k]
        vconj[k] = np.conj(v)
        for g in (0, 1):
            P = pilot_subcarriers(F, g)
            if not len(P):
                continue
            Rfp, Rpp, s2 = R_f[:, P], R_f[np.ix_(P, P)], sigma2
            if despread_f:
                S = np.kron(np.eye(len(P) // 2), [[0.5, 0.5]])
                Rfp, Rpp, s2 = Rfp @ S.T, S @ Rpp @ S.T, sigma2 / 2.0
            W = np.linalg.solve(Rpp + (s2 / lam[k]) * np.eye(Rpp.shape[0]), Rfp.conj().T).conj().T
            filt[g, k, :, :len(P)] = np.repeat(W, 2, axis=1) / 2.0 if despread_f else W
            q = np.real(np.sum(W * np.conj(Rfp), axis=1))                     # [F]
            err[g] -= lam[k] * q[:, None] * (np.abs(tcoef[k]) ** 2)[None, :]
    for g in (0, 1):
        if not len(pilot_subcarriers(F, g)):
            err[g] = R_f[0, 0].real
    ri = lambda z: np.ascontiguousarray(np.stack([z.real, z.imag], -1).astype(dtype))  # noqa: E731
    return LMMSEDesign(ri(filt), ri(tcoef), ri(vconj), err, float(no))


LMMSE3_TABLES = ("qh", "gf", "nu", "tcoef", "vconj", "lam", "vs", "mu")


@dataclasses.dataclass
class LMMSE3Design:
    """Tables of ``nrx_chest_lmmse3`` (include/nrx.h).  They do not depend on ``no``;
    ``err_var(no)`` is the theoretical error map."""
    qh: np.ndarray          # [2, Pmax, Pmax, 2] f32: rows of Q_g^H, qh[g][q][p] = conj(Q_g[p][q])
    gf: np.ndarray          # [2, F, Pmax, 2] f32: G_g = R_f[:, P_g] Q_g
    nu: np.ndarray          # [2, Pmax] f32: eigenvalues of R_f[P_g, P_g]
    tcoef: np.ndarray       # [nd, 14, 2] f32: (R_t[:, D] v_k)[t]
    vconj: np.ndarray       # [nd, nd, 2] f32: conj(v_k[d])
    lam: np.ndarray         # [nd] f32: eigenvalues of R_t[D, D]
    vs: np.ndarray          # [A, A, 2] f32: V_s[a][j]
    mu: np.ndarray          # [A] f32: eigenvalues of R_s
    prior: np.ndarray       # [A] f64: prior variance of an RE of antenna a, R_s[a, a] R_f[0, 0]
    exact: dict             # the unrounded complex128 / float64 tables, for err_var

    def err_var(self, no: float) -> np.ndarray:
        """``E |h - h^|^2`` [2, A, F, 14] float64 per RE of a user of CDM group 0 / 1 at noise ``no``:
        ``prior - sum_{j,k,q} |V_s[a][j] tcoef[k][t] G_g[f][q]|^2 mu_j^2 / (mu_j lambda_k nu_q +
        sigma^2)``, from the unrounded tables (the diagonal of ``C - W C_obs^H`` of the Kronecker
        form; tests/test_chest3_ref.py)."""
        if not no > 0:
            raise ValueError("no must be > 0")
        x = self.exact
        sigma2 = float(no) / 2.0
        vs2, tc2 = np.abs(x["vs"]) ** 2, np.abs(x["tcoef"]) ** 2           # [A, j], [k, T]
        mu, lam = x["mu"], x["lam"]
        err = np.empty((2, len(mu), x["gf"].shape[1], NUM_SYMBOLS))
        for g in (0, 1):
            g2 = np.abs(x["gf"][g]) ** 2                                    # [F, q]
            gain = mu[:, None, None] ** 2 / (mu[:, None, None] * lam[None, :, None] * x["nu"][g][None, None, :]
                                             + sigma2)                      # [j, k, q]
            err[g] = self.prior[:, None, None] - np.einsum("aj,kt,fq,jkq->aft", vs2, tc2, g2, gain)
        return err


def lmmse3_design(R_f: np.ndarray, R_t: np.ndarray, R_s: np.ndarray, params: GenParams,
                  dtype=np.float32) -> LMMSE3Design:
    """The exact Wiener filter under ``R_s (x) R_t (x) R_f`` for LS estimates at the own pilots with
    white noise ``sigma^2 = no / 2``, in the three eigenbases (include/nrx.h nrx_chest_lmmse3):

        R_s = V_s diag(mu) V_s^H  (scaled to trace A),   R_t[D, D] = V_t diag(lambda) V_t^H  (R_t scaled
        to a unit diagonal),   R_f[P_g, P_g] = Q_g diag(nu_g) Q_g^H,   G_g = R_f[:, P_g] Q_g,
        tcoef[k] = R_t[:, D] v_k

        w[j,k,q] = sum_a conj(V_s[a][j]) sum_d conj(V_t[d][k]) sum_p conj(Q_g[p][q]) h_ls[a, P_p, D_d]
        c[j,k,q] = mu_j / (mu_j lambda_k nu_q + sigma^2) w[j,k,q]
        h^[a,f,t] = sum_j V_s[a][j] sum_k tcoef[k][t] sum_q G_g[f][q] c[j,k,q]

    The cross-covariance of ``h`` with the pilots in the eigenbasis is ``(V_s mu) (x) tcoef (x) G_g``
    and the pilots' covariance there is ``diag(mu_j lambda_k nu_q + sigma^2)``, which gives the
    above; it equals the brute-force Kronecker solve (tests/test_chest3_ref.py).  No eigenvalue is
    inverted, so no component is dropped, and ``no`` enters only through the gain: one design serves
    an Eb/N0 sweep.  With ``R_s = I`` the estimate is the 2-D filter of ``lmmse_design``.  Eigenvalues
    that rounding made negative are set to 0.  The tables are rounded once to float32
    (``dtype=np.float64`` keeps them unrounded, for checks)."""
    F, T, A = params.num_subcarriers, NUM_SYMBOLS, params.num_rx_ant
    D = list(params.dmrs_symbols)
    nd = len(D)
    R_f = np.asarray(R_f, np.complex128)
    R_t = np.asarray(R_t, np.complex128)
    R_s = np.asarray(R_s, np.complex128)
    if R_f.shape != (F, F) or R_t.shape != (T, T) or R_s.shape != (A, A):
        raise ValueError(f"R_f must be {(F, F)}, R_t {(T, T)} and R_s {(A, A)}")
    R_t = R_t / R_t[0, 0].real
    R_s = R_s * (A / np.trace(R_s).real)
    mu, Vs = np.linalg.eigh(0.5 * (R_s + R_s.conj().T))
    lam, Vt = np.linalg.eigh(R_t[np.ix_(D, D)])
    mu, lam = np.maximum(mu, 0.0), np.maximum(lam, 0.0)
    Pmax = (F + 1) // 2
    qh = np.zeros((2, Pmax, Pmax), np.complex128)
    gf = np.zeros((2, F, Pmax), np.complex128)
    nu = np.zeros((2, Pmax))
    for g in (0, 1):
        P = pilot_subcarriers(F, g)
        if not len(P):
            continue
        n, Q = np.linalg.eigh(R_f[np.ix_(P, P)])
        nu[g, :len(P)] = np.maximum(n, 0.0)
        qh[g, :len(P), :len(P)] = Q.conj().T
        gf[g, :, :len(P)] = R_f[:, P] @ Q
    tcoef = (R_t[:, D] @ Vt).T                                              # [k, T]
    vconj = Vt.conj().T                                                     # [k, d]
    ri = lambda z: np.ascontiguousarray(np.stack([z.real, z.imag], -1).astype(dtype))  # noqa: E731
    re = lambda x: np.ascontiguousarray(x.astype(dtype))                    # noqa: E731
    exact = dict(gf=gf, nu=nu, tcoef=tcoef, lam=lam, vs=Vs, mu=mu)
    return LMMSE3Design(ri(qh), ri(gf), re(nu), ri(tcoef), ri(vconj), re(lam), ri(Vs), re(mu),
                        prior=np.real(np.diag(R_s)) * R_f[0, 0].real, exact=exact)


class ChannelEstimator:
    """``est(sb, no) -> h_est [B, U, F, 14, 2A]``: ``"lin"`` (``nrx_chest_lin``), ``"lmmse"``
    (``nrx_chest_lmmse``) or ``"lmmse3"`` (``nrx_chest_lmmse3``) on the LS estimates that
    ``sb.h_hat`` holds at the own pilots.  ``"lmmse"`` needs the covariance (``R_f``, ``R_t`` here or
    ``set_covariance``) and designs its filter whenever ``no`` changes (``self.design``);
    ``"lmmse3"`` needs ``R_s`` as well and designs once per covariance.  ``tables=`` pins given
    ``LMMSEDesign`` / ``LMMSE3Design`` tables instead.  Every element of the output is written;
    inactive users are 0.  ``cfo`` (a ``cfo.CFOCompensator``, here or per call): every call
    estimates the carrier frequency offset, de-rotates the pilots, estimates, and re-rotates the
    output (``CFOCompensator.wrap``)."""

    def __init__(self, kind: str, params: GenParams, device: int = 0, R_f=None, R_t=None,
                 tables=None, R_s=None, cfo=None):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.kind = kind
        self.p = params
        self.device = device
        self.cfo = cfo
        # cover-coded ports (GenParams.dmrs): h_hat holds despread estimates.  A frequency pair holds one
        # value, which lin interpolates as it is and lmmse designs its filter for; the rest is out of scope
        self.despread_f = params.dmrs is not None and params.dmrs.despread_f
        if params.dmrs is not None and params.dmrs.despread_t:
            raise ValueError(f"the {kind} estimator does not take time-despread pilots (ports with a time cover): "
                             "the two symbols of a pair hold one estimate")
        if self.despread_f and kind == "lmmse3":
            raise ValueError("the 3-D LMMSE estimator is not designed for cover-coded DMRS ports: use the 2-D "
                             "filter (evaluate: -chest_2d)")
        self._lib = _lib.load()
        self.R_f, self.R_t, self.R_s = R_f, R_t, R_s
        self.design = None
        self._pinned = tables is not None
        self._dev = None
        self._out = None
        self._ws = Workspace()
        self.last_workspace_bytes = 0      # what nrx_chest3_workspace_size asked for the last call
        if tables is not None:
            self._set_design(tables)

    def set_covariance(self, R_f, R_t, R_s=None) -> None:
        self.R_f, self.R_t, self.R_s = R_f, R_t, R_s
        if not self._pinned:
            self.design = None

    def _set_design(self, d) -> None:
        p = self.p
        nd, F, A = len(p.dmrs_symbols), p.num_subcarriers, p.num_rx_ant
        Pmax = (F + 1) // 2
        if self.kind == "lmmse3":
            shapes = dict(qh=(2, Pmax, Pmax, 2), gf=(2, F, Pmax, 2), nu=(2, Pmax), tcoef=(nd, NUM_SYMBOLS, 2),
                          vconj=(nd, nd, 2), lam=(nd,), vs=(A, A, 2), mu=(A,))
            if not isinstance(d, LMMSE3Design) or any(
                    getattr(d, k).shape != s or getattr(d, k).dtype != np.float32 for k, s in shapes.items()):
                raise ValueError("tables do not match the parameters (lmmse3_design)")
        elif d.filt.shape != (2, nd, F, Pmax, 2) or d.tcoef.shape != (nd, NUM_SYMBOLS, 2) \
                or d.vconj.shape != (nd, nd, 2) or any(a.dtype != np.float32 for a in (d.filt, d.tcoef, d.vconj)):
            raise ValueError("tables do not match the parameters (lmmse_design)")
        self.design = d
        self._dev = None            # uploaded by the next call

    def prepare(self, no: float):
        """(re-)design the LMMSE filter for ``no``; the design in use"""
        if self.kind == "lin" or self._pinned:
            return self.design
        if self.kind == "lmmse3":
            if self.design is None:
                if self.R_f is None or self.R_t is None or self.R_s is None:
                    raise ValueError("the 3-D LMMSE estimator needs R_f, R_t and R_s (set_covariance)")
                self._set_design(lmmse3_design(self.R_f, self.R_t, self.R_s, self.p))
            return self.design
        if self.design is None or self.design.no != float(no):
            if self.R_f is None or self.R_t is None:
                raise ValueError("the LMMSE estimator needs the covariance matrices (set_covariance)")
            self._set_design(lmmse_design(self.R_f, self.R_t, self.p, no, despread_f=self.despread_f))
        return self.design

    def __call__(self, sb: SlotBatch, no: float, out=None, stream=None, workspace=None, cfo=None):
        """``workspace`` (lmmse3 only, the one estimator with a workspace): a uint8 device tensor
        of at least ``nrx_chest3_workspace_size`` bytes (``last_workspace_bytes`` after a call),
        any content, instead of the estimator's own.  ``cfo``: a ``cfo.CFOCompensator`` for this
        call, None for the estimator's own (``self.cfo``), False for none."""
        cfo = self.cfo if cfo is None else cfo
        if cfo:
            return cfo.wrap(self)(sb, no, out=out, stream=stream, workspace=workspace)
        torch = _torch()
        p = self.p
        hh = sb.h_hat
        if hh is None:
            raise ValueError("the slot batch has no h_hat")
        B = hh.shape[0]
        shape = (B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, 2 * p.num_rx_ant)
        require("h_hat", hh, shape, torch.float32, f"cuda:{self.device}")
        require("active", sb.active, (B, p.num_tx), torch.float32)
        if out is None:
            if self._out is None or self._out.shape[0] != B:
                self._out = torch.empty(shape, dtype=torch.float32, device=hh.device)
            out = self._out
        else:
            require("out", out, shape, torch.float32)
        if workspace is not None and self.kind != "lmmse3":
            raise ValueError(f"the {self.kind} estimator takes no workspace")
        # nrx_chest_io and nrx_chest3_io differ in their tables only
        io = _lib.nrx_chest3_io() if self.kind == "lmmse3" else _lib.nrx_chest_io()
        fill_grid(io, *shape[:4], p.num_rx_ant)
        fill_dmrs(io, p.dmrs_symbols, p.cdm_group, p.num_tx)
        io.no = float(no)
        io.h_hat, io.active, io.h_out = ptr(hh), ptr(sb.active), ptr(out)
        stream = stream_of(hh, stream)
        if self.kind == "lin":
            _lib.check(self._lib.nrx_chest_lin(ref(io), stream))
            return out
        d = self.prepare(no)
        tables = LMMSE3_TABLES if self.kind == "lmmse3" else ("filt", "tcoef", "vconj")
        if self._dev is None:
            self._dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(d, k))).to(hh.device) for k in tables}
        for k in tables:
            setattr(io, k, self._dev[k].data_ptr())
        if self.kind == "lmmse":
            _lib.check(self._lib.nrx_chest_lmmse(ref(io), stream))
            return out
        self.last_workspace_bytes = self._ws.size(self._lib.nrx_chest3_workspace_size, ref(io))
        ws = self._ws.get(self.last_workspace_bytes, out.device, workspace)
        _lib.check(self._lib.nrx_chest_lmmse3(ref(io), ws.data_ptr(), ws.numel(), stream))
        return out


class EstimatorBaselineReceiver(Receiver):
    """``rx(sb, no) -> llr [1, B, U, F, T, bits_max]`` for ``baseline_lslin_lmmse`` (linear
    interpolation) and ``baseline_lmmse_lmmse`` (2-D LMMSE estimation; needs ``R_f`` / ``R_t`` from
    a ``CovarianceEstimator``, here or through ``set_covariance``), both followed by the LMMSE
    detector of ``baseline.LMMSEDetector``.  Same call signature and ``contaminated`` property as
    ``baseline.BaselineReceiver``, and the same limit: both work on LS estimates at the pilots, so
    they are meaningful for at most one active port per CDM group -- or for cover-coded ports
    (``GenParams.dmrs``), whose despread estimates separate the ports of a group: lin runs unchanged on
    them, lmmse designs its filter for them (``lmmse_design(despread_f=True)``).  Refused: the 3-D
    filter under cover codes, and every estimator on time-despread pilots.

    The detector takes one scalar ``err_var`` where Sionna passes a per-RE map -- an approximation
    in both systems: lmmse passes ``num_active x`` the mean over users' groups, subcarriers and data
    symbols of the theoretical error map of the design; lin passes ``num_active * no / 2``, the LS
    error at a pilot, as ``baseline_lsnn_lmmse`` does."""

    SYSTEMS = SYSTEMS

    def __init__(self, system: str, params: GenParams, device: int = 0, R_f=None, R_t=None, R_s=None, cfo=None):
        super().__init__(system, params, device)
        self._device = device
        self.cfo = cfo          # a cfo.CFOCompensator the estimator runs through, or None
        self.estimator = None
        self._ev3 = None
        self.set_covariance(R_f, R_t, R_s)

    def set_covariance(self, R_f, R_t, R_s=None) -> None:
        """``R_s=None`` keeps the 2-D filter; a matrix selects the 3-D one (``baseline_lmmse_lmmse`` only)"""
        kind = "lin" if self.system != "baseline_lmmse_lmmse" else "lmmse" if R_s is None else "lmmse3"
        if self.estimator is None or self.estimator.kind != kind:
            self.estimator = ChannelEstimator(kind, self.p, self._device, cfo=self.cfo)
        if kind == "lmmse3":
            self.estimator.set_covariance(R_f, R_t, R_s)
        else:
            self.estimator.set_covariance(R_f, R_t)

    def err_var(self, no: float) -> float:
        if self.estimator.kind == "lin":     # the LS error at a pilot, over the despreading block
            return self._num_active * float(no) / (2.0 * (2 if self.estimator.despread_f else 1))
        d = self.estimator.prepare(no)
        data = [t for t in range(NUM_SYMBOLS) if t not in self.p.dmrs_symbols]
        groups = list(self.p.cdm_group[:self.p.num_tx])
        if self.estimator.kind == "lmmse3":     # the design does not depend on no: the map is cached per no
            if self._ev3 is None or self._ev3[0] is not d or self._ev3[1] != float(no):
                ev = d.err_var(no)              # [2, A, F, 14]: also the mean over the antennas
                self._ev3 = (d, float(no), self._num_active * float(np.mean([ev[g][:, :, data].mean() for g in groups])))
            return self._ev3[2]
        return self._num_active * float(np.mean([d.err_var[g][:, data].mean() for g in groups]))

    def _estimate(self, sb: SlotBatch, no: float, stream):
        return self.estimator(sb, no, stream=stream)


def estimate_covariance(gen, num_slots: int, batch_size: int, no: float = 1.0,
                        slot_offset: int = COV_SLOT_OFFSET) -> CovarianceEstimator:
    """Accumulate the covariance over ``num_slots`` generated slots starting at ``slot_offset``
    (default 2^40, beyond every Monte-Carlo offset), as the reference runs compute_cov_mat.py before
    an evaluation.  The true channel does not depend on ``no``.  ``gen`` needs ``want_h=True``."""
    if not gen.want_h:
        raise ValueError("the covariance needs SlotGenerator(want_h=True)")
    cov = CovarianceEstimator(gen.p, gen.device)
    done = 0
    while done < num_slots:
        b = min(batch_size, num_slots - done)
        cov.accumulate(gen(b, no, slot_offset=slot_offset + done))
        done += b
    return cov
