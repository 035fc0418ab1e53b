"""Seeded PUSCH slot generator and uncoded error counters on the GPU.

Mirrors the data side of the reference's ``E2E_Model.forward``
(utils/e2e_model.py:219-344): random active DMRS ports (``_active_dmrs_mask``, 187-193),
bits -> Gray QAM on a DMRS type-1 resource grid, channel + AWGN at an Eb/N0-derived noise
variance (323-332), LS channel estimate -> the CGNN's inputs; and the counting side of
``sim_ber`` with ``_mask_active_dmrs`` (195-209).  Sionna's UMi channel and LDPC chain
are not available here; the generator's channel is the seeded tapped-delay line stated in
``oracle/synth_ref.py`` and the counters are uncoded (hard decisions on the LLRs).

``GenParams.user_profiles`` / ``rx_corr`` (and ``scenario``) add what the reference's evaluation
channel ``DoubleTDL`` defines in its own text: a delay and Doppler spread per user and gNB antenna
correlation (utils/channel_models.py:20-161), through ``nrx_generate_slots_ex``.

Everything runs through ``libnrx.so`` (``nrx_generate_slots`` / ``nrx_generate_slots_ex`` /
``nrx_count_errors``, include/nrx.h); torch tensors are only device containers.

``GenParams.cfo_hz`` adds a per-user carrier frequency offset at the transmitter (the reference's
``cfo_offset_ppm(_eval)``, utils/impairments.py:18-110), through ``nrx_generate_slots_cfo``; the
receiver-side remedy is ``neural_rx_amd/cfo.py``.

``GenParams.dmrs`` (an ``ls.DMRSPorts``) gives the ports orthogonal cover codes, through
``nrx_generate_slots_dmrs``: ``h_hat`` and the Aerial pilot list are then the despreading LS estimate
of ``neural_rx_amd/ls.py`` and ``SlotBatch.pilots`` is the pilot table an external caller of it needs.

``GenParams.cir`` (a ``cir.CIRChannel``) replaces the tapped-delay line by a replayed set of channel impulse
responses, through ``nrx_generate_slots_cir``; ``SlotGenerator.export_taps`` writes the built-in channel in
that format (``nrx_generate_taps``).

``GenParams.td`` (a ``TimeDomain``) puts a time-domain transmit stage between the transmit grid and the channel,
``x' = demodulate(impair(modulate(x)))`` through ``nrx_generate_slots_td``: a per-user timing error and a Rapp
power amplifier, the two transmit-side effects without a closed form on the grid (the construction of the
reference's utils/impairments.py:67-108; the transforms are those of ``neural_rx_amd/ofdm.py``).

``GenParams.tc`` (a ``TimeChannelParams``) replaces the per-RE channel product by the time-domain channel of
``neural_rx_amd/timechannel.py`` between modulation and demodulation, through ``nrx_generate_slots_tc``: path
gains that move inside a symbol (inter-carrier interference) and delay taps that may exceed the cyclic prefix
(inter-symbol interference), with the built-in channel's own draws, so a run with zero Doppler is the plain
generator's realisation up to the truncation of the sinc taps.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._call import Workspace, fill_dmrs, fill_grid, fill_mcs, ptr, ref, require, stream_of, torch as _torch
from .cir import SELECT, CIRChannel, CIRDataset
from .config import NRXConfig, dmrs_symbols, get_config, user_cdm_groups
from .ls import DMRSPorts
from .ofdm import default_cp

NUM_SYMBOLS = 14


def ebno_to_no(ebno_db: float, num_dmrs_symbols: int = 2, num_symbols: int = NUM_SYMBOLS) -> float:
    """Rate-adjusted SNR of the torch E2E model (e2e_model.py:323-332, ``ebno = True`` in
    nrx_rt.cfg:13): ``ebno_db -= 10 log10(1 - pilots / REs)``; ``no = 10^(-ebno_db / 10)``.
    With two CDM groups without data every RE of a DMRS symbol is a pilot RE."""
    ebno_db = ebno_db - 10.0 * np.log10(1.0 - num_dmrs_symbols / num_symbols)
    return float(10.0 ** (-ebno_db / 10.0))


@dataclasses.dataclass
class TimeDomain:
    """The time-domain transmit stage (include/nrx.h nrx_gen_td).  ``delay``: samples by which each port's
    signal arrives late, one value or one per port; ``pa_ibo_db``: the Rapp amplifier's input back-off over the
    nominal mean sample power F / N, None = a linear amplifier; ``h_with_delay``: ``SlotBatch.h`` carries the
    delay's frequency ramp, the effective channel a perfect-CSI receiver should be scored against."""
    fft_size: int
    cp: Optional[object] = None        # one int or 14; None = ofdm.default_cp(fft_size)
    delay: object = 0
    pa_ibo_db: Optional[float] = None
    pa_smoothness: float = 2.0
    h_with_delay: bool = False
    first_bin: int = -1

    def cp_list(self) -> list:
        cp = default_cp(self.fft_size) if self.cp is None else self.cp
        v = [int(c) for c in np.atleast_1d(cp)]
        if len(v) == 1:
            v = v * NUM_SYMBOLS
        if len(v) != NUM_SYMBOLS:
            raise ValueError(f"cp needs one value or one per symbol: {NUM_SYMBOLS}, got {len(v)}")
        return v

    def delay_per_port(self, num_tx: int) -> list:
        v = [int(d) for d in np.atleast_1d(self.delay)]
        if len(v) == 1:
            v = v * num_tx
        if len(v) != num_tx:
            raise ValueError(f"delay needs one value or one per port: {num_tx}, got {len(v)}")
        return v

    def struct(self, num_tx: int) -> _lib.nrx_gen_td:
        t = _lib.nrx_gen_td()
        t.fft_size, t.first_bin = int(self.fft_size), int(self.first_bin)
        for k, c in enumerate(self.cp_list()):
            t.cp_length[k] = c
        for u, d in enumerate(self.delay_per_port(num_tx)[:16]):
            t.delay[u] = d
        t.pa_enable, t.h_with_delay = int(self.pa_ibo_db is not None), int(self.h_with_delay)
        t.pa_ibo_db = 0.0 if self.pa_ibo_db is None else float(self.pa_ibo_db)
        t.pa_smoothness = float(self.pa_smoothness)
        return t


@dataclasses.dataclass
class TimeChannelParams:
    """The time-domain channel of the generator (include/nrx.h nrx_gen_tc).  Taps ``l_min..l_max`` of the plainly
    truncated sinc (``l_max = None``: the longest port delay in samples, rounded up, + 6); ``timing_advance``:
    the receive windows start this many samples early (0..min cp).  ``SlotBatch.h`` is then the ISI-free
    diagonal of the effective channel: exact when ``l_max <= cp - timing_advance`` and ``timing_advance >=
    -l_min``, the dominant term otherwise."""
    fft_size: int
    cp: Optional[object] = None        # one int or 14; None = ofdm.default_cp(fft_size)
    l_min: int = -6
    l_max: Optional[int] = None
    timing_advance: int = 0
    first_bin: int = -1

    def cp_list(self) -> list:
        return TimeDomain.cp_list(self)

    def num_samples(self) -> int:
        return sum(c + int(self.fft_size) for c in self.cp_list())

    def struct(self) -> _lib.nrx_gen_tc:
        t = _lib.nrx_gen_tc()
        t.fft_size, t.first_bin = int(self.fft_size), int(self.first_bin)
        for k, c in enumerate(self.cp_list()):
            t.cp_length[k] = c
        t.l_min, t.l_max = int(self.l_min), -1 if self.l_max is None else int(self.l_max)
        t.timing_advance = int(self.timing_advance)
        return t


@dataclasses.dataclass
class GenParams:
    """Everything that defines a batch of generated slots (besides ``no``/offset)."""
    num_tx: int
    num_subcarriers: int
    num_rx_ant: int
    dmrs_symbols: Sequence[int] = (2, 11)
    cdm_group: Sequence[int] = (0, 1)
    mcs_bits: Sequence[int] = (4,)
    mcs_of_user: Optional[Sequence[int]] = None    # per port; -1 = drawn per slot
    num_active: Optional[int] = None               # None = all ports active
    num_taps: int = 6
    num_sinusoids: int = 4
    max_delay_s: float = 300e-9
    max_doppler_hz: float = 400.0
    subcarrier_spacing: float = 30e3
    seed: int = 1234
    # per port (max_delay_s, max_doppler_hz), replacing the two scalars above; None = the scalars
    user_profiles: Optional[Sequence] = None
    # receive-antenna correlation, A x A Hermitian PSD (rx_correlation); None = i.i.d. antennas
    rx_corr: Optional[np.ndarray] = None
    # carrier frequency offset in Hz, one value or one per port (include/nrx.h nrx_gen_cfo); None = the
    # generator without it.  Drawn uniformly in +-cfo_hz per (slot, user) unless cfo_constant.
    cfo_hz: Optional[object] = None
    cfo_constant: bool = False
    fft_size: int = 0                  # N of the CFO's Dirichlet kernel; 0 = num_subcarriers
    h_with_phase: bool = False         # SlotBatch.h = the diagonal of the effective channel under the CFO
    # cover-coded DMRS ports (ls.DMRSPorts; its cdm_group replaces the one above); None = the generator
    # without cover codes, where every port draws its own pilots
    dmrs: Optional[DMRSPorts] = None
    # a replayed channel-impulse-response dataset (cir.CIRChannel) in place of the tapped-delay line; None =
    # the built-in channel.  Excludes user_profiles / rx_corr: a dataset brings its own structure.
    cir: Optional[CIRChannel] = None
    # a time-domain transmit stage (TimeDomain): per-user timing error and power amplifier; None = the generator
    # without it.  Excludes cfo_hz: one transmit-side stage per generator.
    td: Optional[TimeDomain] = None
    # the time-domain channel (TimeChannelParams) in place of the per-RE product; None = the grid channel.
    # Excludes td, cir and cfo_hz: one sample-domain stage per generator.  dmrs composes: it acts on x.
    tc: Optional[TimeChannelParams] = None

    def __post_init__(self):
        if self.tc is not None and (self.td is not None or self.cir is not None or self.cfo_hz is not None):
            raise ValueError("tc with td, cir or cfo_hz: a generator takes one sample-domain stage "
                             "(as it takes one transmit-side stage)")
        if self.td is not None and self.cfo_hz is not None:
            raise ValueError("td and cfo_hz are two transmit-side stages: a generator takes one of them")
        if self.cir is not None:
            if self.user_profiles is not None or self.rx_corr is not None:
                raise ValueError("a cir dataset is the channel: user_profiles and rx_corr do not apply to it")
            if self.cir.dataset.num_rx_ant != self.num_rx_ant:
                raise ValueError(f"the cir dataset has {self.cir.dataset.num_rx_ant} antennas, num_rx_ant is "
                                 f"{self.num_rx_ant}")
            if self.cir.select == "trajectory" and self.cir.dataset.num_examples < self.num_tx:
                raise ValueError("select='trajectory' needs at least one example per user")
        if self.dmrs is not None:
            if self.dmrs.num_tx != self.num_tx:
                raise ValueError(f"dmrs holds {self.dmrs.num_tx} ports, num_tx is {self.num_tx}")
            self.dmrs.validate(self.num_subcarriers, self.dmrs_symbols)
            self.cdm_group = tuple(self.dmrs.cdm_group)

    @classmethod
    def from_config(cls, cfg: NRXConfig | str, num_tx: Optional[int] = None, num_prbs: Optional[int] = None,
                    num_rx_ant: Optional[int] = None, var_mcs: bool = False, **kw) -> "GenParams":
        """Generator parameters for a reference config: its DMRS symbols and ports
        (config.dmrs_symbols / user_cdm_groups), its MCS list (``mcs_index``; with
        ``var_mcs`` the MCS of each (slot, user) is drawn, as the var-MCS evaluation's
        random ``mcs_ue_mask``), its PRBs and antennas."""
        if isinstance(cfg, str):
            cfg = get_config(cfg)
        u = num_tx or cfg.max_num_tx
        return cls(num_tx=u, num_subcarriers=12 * (num_prbs or cfg.n_size_bwp),
                   num_rx_ant=num_rx_ant or cfg.num_rx_antennas, dmrs_symbols=dmrs_symbols(cfg),
                   cdm_group=user_cdm_groups(cfg, u), mcs_bits=cfg.bits_per_head,
                   mcs_of_user=[-1] * u if var_mcs else [0] * u, **kw)

    @property
    def bits_max(self) -> int:
        return max(self.mcs_bits)

    def desc(self, batch: int, no: float, slot_offset: int = 0) -> _lib.nrx_gen_desc:
        d = _lib.nrx_gen_desc()
        fill_grid(d, batch, self.num_tx, self.num_subcarriers, NUM_SYMBOLS, self.num_rx_ant)
        fill_dmrs(d, self.dmrs_symbols, self.cdm_group, self.num_tx)
        fill_mcs(d, self.mcs_bits, self.dmrs_symbols)
        if self.mcs_of_user is not None:
            for u in range(min(self.num_tx, 16)):
                d.mcs_of_user[u] = self.mcs_of_user[u]
        d.num_active = self.num_tx if self.num_active is None else self.num_active
        d.num_taps, d.num_sinusoids = self.num_taps, self.num_sinusoids
        d.max_delay_s, d.max_doppler_hz = self.max_delay_s, self.max_doppler_hz
        d.subcarrier_spacing, d.no = self.subcarrier_spacing, no
        d.seed, d.slot_offset = self.seed, slot_offset
        return d

    @property
    def correlated(self) -> bool:
        """the slots need ``nrx_generate_slots_ex``"""
        return self.user_profiles is not None or self.rx_corr is not None

    def profiles(self) -> list:
        """(max_delay_s, max_doppler_hz) of every port"""
        if self.user_profiles is None:
            return [(float(self.max_delay_s), float(self.max_doppler_hz))] * self.num_tx
        prof = [(float(a), float(b)) for a, b in self.user_profiles]
        if len(prof) != self.num_tx:
            raise ValueError(f"user_profiles needs one (max_delay_s, max_doppler_hz) per port: "
                             f"{self.num_tx}, got {len(prof)}")
        return prof

    def cfo_per_port(self) -> Optional[list]:
        """``cfo_hz`` of every port, or None"""
        if self.cfo_hz is None:
            return None
        v = [float(x) for x in np.atleast_1d(np.asarray(self.cfo_hz, np.float64))]
        if len(v) == 1:
            v = v * self.num_tx
        if len(v) != self.num_tx:
            raise ValueError(f"cfo_hz needs one value or one per port: {self.num_tx}, got {len(v)}")
        return v

    def rx_mix(self) -> Optional[np.ndarray]:
        """``M = V diag(sqrt(mu)) V^H``, the Hermitian square root of ``rx_corr`` (complex128
        [A, A], ``M M^H = rx_corr``), or None.  Eigenvalues below zero by rounding count as 0."""
        if self.rx_corr is None:
            return None
        A = self.num_rx_ant
        R = np.asarray(self.rx_corr, np.complex128)
        if R.shape != (A, A) or not np.allclose(R, R.conj().T, rtol=0, atol=1e-12 * max(1.0, np.abs(R).max())):
            raise ValueError(f"rx_corr must be a Hermitian {(A, A)} matrix")
        mu, V = np.linalg.eigh(R)
        if mu[0] < -1e-9 * max(mu[-1], 1e-300):
            raise ValueError("rx_corr must be positive semi-definite")
        return (V * np.sqrt(np.maximum(mu, 0.0))) @ V.conj().T


def rx_correlation(num_rx_ant: int, alpha: float) -> np.ndarray:
    """Receive-antenna correlation ``R[i][j] = alpha^((|i - j| / (A - 1))^2)`` (A = 1: ``[[1]]``),
    float64 [A, A].  For A in {2, 4, 8} these are the exponent tables of the reference's
    ``gnb_correlation_matrix`` (utils/channel_models.py:20-33; alpha = 0 / 0.9 for low / high
    correlation, 96-107); the closed form extends them to any A.  It is a Gaussian kernel in the antenna index, hence positive semi-definite."""
    A = int(num_rx_ant)
    if A < 1:
        raise ValueError("num_rx_ant must be >= 1")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must be in [0, 1]")
    if A == 1:
        return np.ones((1, 1))
    i = np.arange(A)
    e = (np.abs(i[:, None] - i[None, :]) / (A - 1.0)) ** 2
    return np.where(e == 0, 1.0, float(alpha) ** e)


# rms delay spread of the generator's delay profile over its max_delay_s (scenario docstring)
RMS_OVER_MAX_DELAY = 0.23658
SCENARIOS = {"double_tdl_low": 0.0, "double_tdl_high": 0.9}
DOUBLE_TDL_USERS = ((100e-9, 400.0), (300e-9, 100.0))     # (rms delay spread, max Doppler) of port 0 / 1


def scenario(name: str, params: GenParams) -> GenParams:
    """``params`` on the reference's evaluation channel ``DoubleTDL`` (utils/channel_models.py:
    39-161, ``channel_type_eval = "DoubleTDLlow"``): two users with different profiles -- port 0
    delay spread 100 ns / 400 Hz Doppler, port 1 300 ns / 100 Hz -- and gNB antenna correlation
    ``rx_correlation(A, alpha)``, alpha = 0 (``"double_tdl_low"``) or 0.9 (``"double_tdl_high"``).
    It needs exactly two ports, as the reference's scripts/evaluate.py:177-180 does.

    Delay spread.  The generator draws delays uniformly on [0, max] and weighs them by
    exp(-3 tau / max), so its continuous PDP is p(x) ~ exp(-3 x) on x = tau / max in [0, 1]:
    m0 = (1 - e^-3) / 3, E x = (1/9 - 4/9 e^-3) / m0 = 0.280936, E x^2 = (2/27 - 17/27 e^-3) / m0 =
    0.134897, so the rms delay spread is sqrt(E x^2 - (E x)^2) max = 0.23658 max and
    ``max_delay_s = DS / 0.23658``.

    Two stated departures: the taps are still the generator's random ones (uniform delays,
    sum-of-sinusoids Doppler), not the 3GPP TDL-B / TDL-C tables; and the reference's "medium"
    correlation differs from "high" only on the UE side, which has one antenna here, so there is no
    separate preset."""
    if name not in SCENARIOS:
        raise ValueError(f"scenario must be one of {tuple(SCENARIOS)}, got {name!r}")
    if params.num_tx != 2:
        raise ValueError(f"the DoubleTDL scenarios are defined for exactly two ports, got {params.num_tx}")
    prof = [(ds / RMS_OVER_MAX_DELAY, fd) for ds, fd in DOUBLE_TDL_USERS]
    return dataclasses.replace(params, user_profiles=prof, rx_corr=rx_correlation(params.num_rx_ant, SCENARIOS[name]))


@dataclasses.dataclass
class SlotBatch:
    """Device tensors of one generated batch (CGNN layout, include/nrx.h)."""
    y: "object"            # [B, F, T, 2A] f32
    h_hat: "object"        # [B, U, F, T, 2A] f32
    active: "object"       # [B, U] f32
    mcs_mask: "object"     # [B, U, M] f32
    mcs: "object"          # [B, U] u8
    bits: "object"         # [B, U, F, T, bits_max] u8
    h: "object" = None     # [B, U, F, T, 2A] f32 (true channel) or None
    y_real: "object" = None
    y_imag: "object" = None
    h_ls_real: "object" = None
    h_ls_imag: "object" = None
    cfo_eps: "object" = None   # [B, U] f64: the carrier frequency offset in subcarrier spacings, or None
    pilots: "object" = None    # [2, Pmax, nd, 2] f32: the DMRS base sequence (GenParams.dmrs), or None
    x_td: "object" = None      # [B, U, F, T] c128: the grid behind the time-domain stage (GenParams.td), or None
    r_tc: "object" = None      # [B, A, Ls] c128: the noise-free received samples (GenParams.tc), or None


class SlotGenerator:
    """``gen(batch, no, slot_offset) -> SlotBatch`` on one GPU.  Slot ``slot_offset + b``
    is the same slot whichever call, rank or batch split generates it."""

    def __init__(self, params: GenParams, device: int = 0, want_h: bool = False, aerial: bool = False,
                 want_x: bool = False, want_r: bool = False):
        self.p = params
        self.device = device
        self.want_h = want_h
        self.aerial = aerial
        self.want_x = want_x            # SlotBatch.x_td (with GenParams.td)
        self.want_r = want_r            # SlotBatch.r_tc (with GenParams.tc)
        self._lib = _lib.load()
        self._ws = Workspace()
        self._bufs = {}
        self._chan = None
        self._mix = None        # device copy of rx_mix(), uploaded once
        if params.correlated:
            c = _lib.nrx_gen_chan()
            for u, (delay, doppler) in enumerate(params.profiles()):
                c.max_delay_s[u], c.max_doppler_hz[u] = delay, doppler
            M = params.rx_mix()
            if M is not None:
                torch = _torch()
                m = np.ascontiguousarray(np.stack([M.real, M.imag], -1))
                self._mix = torch.from_numpy(m).to(f"cuda:{device}")
                c.rx_mix = self._mix.data_ptr()
            self._chan = c
        self._cfo = None
        if params.cfo_hz is not None:
            c = _lib.nrx_gen_cfo()
            for u, hz in enumerate(params.cfo_per_port()):
                c.cfo_hz[u] = hz
            c.constant, c.fft_size, c.h_with_phase = int(params.cfo_constant), int(params.fft_size), int(params.h_with_phase)
            self._cfo = c
        self._dmrs = None
        if params.dmrs is not None:
            m = _lib.nrx_gen_dmrs()
            for u in range(params.num_tx):
                m.focc[u], m.tocc[u] = params.dmrs.focc[u], params.dmrs.tocc[u]
            m.despread_f, m.despread_t = int(params.dmrs.despread_f), int(params.dmrs.despread_t)
            self._dmrs = m
        self._cir = None
        if params.cir is not None:
            ch = params.cir
            self._cir_data = ch.dataset.to(f"cuda:{device}")       # kept alive: the struct holds its pointers
            r = _lib.nrx_gen_cir()
            r.num_examples, r.num_paths = self._cir_data.num_examples, self._cir_data.num_paths
            r.num_time_steps, r.select = self._cir_data.num_time_steps, SELECT[ch.select]
            r.normalize, r.f_offset = int(bool(ch.normalize)), ch.offset(params.num_subcarriers)
            torch = _torch()
            self._cir_a = torch.view_as_real(self._cir_data.a.contiguous())
            self._cir_tau = self._cir_data.tau.contiguous()
            r.a, r.tau = self._cir_a.data_ptr(), self._cir_tau.data_ptr()
            self._cir = r
        self._td = params.td.struct(params.num_tx) if params.td is not None else None
        self._tc = params.tc.struct() if params.tc is not None else None

    def workspace_bytes(self, batch: int) -> int:
        """what ``nrx_gen_workspace_size_tc`` asks for with whichever blocks this generator has (NULL for
        the absent ones: the older ``nrx_gen_workspace_size*`` are that call with fewer blocks)"""
        if self._cir is not None and self._cir.select == SELECT["index"] and not self._cir.index:
            # the size is no function of the index, which comes with every call: any address passes the check
            self._cir.index = self._cir_tau.data_ptr()
        return self._ws.size(self._lib.nrx_gen_workspace_size_tc, ref(self.p.desc(batch, 0.0)), ref(self._chan),
                             ref(self._cfo), ref(self._dmrs), ref(self._cir), ref(self._td), ref(self._tc))

    def _alloc(self, batch: int) -> SlotBatch:
        torch = _torch()
        key = batch
        if key in self._bufs:
            return self._bufs[key]
        p, dev = self.p, f"cuda:{self.device}"
        U, F, A, M = p.num_tx, p.num_subcarriers, p.num_rx_ant, len(p.mcs_bits)
        f32 = dict(dtype=torch.float32, device=dev)
        sb = SlotBatch(
            y=torch.empty((batch, F, NUM_SYMBOLS, 2 * A), **f32),
            h_hat=torch.empty((batch, U, F, NUM_SYMBOLS, 2 * A), **f32),
            active=torch.empty((batch, U), **f32),
            mcs_mask=torch.empty((batch, U, M), **f32),
            mcs=torch.empty((batch, U), dtype=torch.uint8, device=dev),
            bits=torch.empty((batch, U, F, NUM_SYMBOLS, p.bits_max), dtype=torch.uint8, device=dev),
            h=torch.empty((batch, U, F, NUM_SYMBOLS, 2 * A), **f32) if self.want_h else None)
        if self.aerial:
            npil = len(p.dmrs_symbols) * (F // 12) * 6
            sb.y_real = torch.empty((batch, F, NUM_SYMBOLS, A), **f32)
            sb.y_imag = torch.empty_like(sb.y_real)
            sb.h_ls_real = torch.empty((batch, npil, U, A), **f32)
            sb.h_ls_imag = torch.empty_like(sb.h_ls_real)
        if self._cfo is not None:      # zeros: an all-zero cfo_hz is the generator without it, which writes no eps
            sb.cfo_eps = torch.zeros((batch, U), dtype=torch.float64, device=dev)
        if self._dmrs is not None:
            sb.pilots = torch.empty((2, (F + 1) // 2, len(p.dmrs_symbols), 2), **f32)
        if self._td is not None and self.want_x:
            sb.x_td = torch.empty((batch, U, F, NUM_SYMBOLS), dtype=torch.complex128, device=dev)
        if self._tc is not None and self.want_r:
            sb.r_tc = torch.empty((batch, A, p.tc.num_samples()), dtype=torch.complex128, device=dev)
        self._bufs = {key: sb}
        return sb

    def __call__(self, batch: int, no, slot_offset: int = 0, stream=None, out: Optional[SlotBatch] = None,
                 workspace=None, cir_index=None) -> SlotBatch:
        """``no``: the noise variance per complex resource element, one float for the batch or a float64
        device tensor ``[batch]`` with one value per slot (finite and >= 0: the host never reads it), which
        goes through ``nrx_generate_slots_no``.  ``workspace``: a uint8 device tensor of at least ``workspace_bytes(batch)`` bytes, any
        content, to run this call in instead of the generator's own.  ``cir_index``: the examples
        ``[batch, U]`` int32 (device) of a ``CIRChannel(select="index")``."""
        torch = _torch()
        sb = out if out is not None else self._alloc(batch)
        nbytes = self.workspace_bytes(batch) if workspace is None else 0      # the C call sizes a caller's
        ws = self._ws.get(nbytes, f"cuda:{self.device}", workspace)
        noise = None
        if hasattr(no, "data_ptr"):
            require("no", no, (batch,), torch.float64, sb.y.device)
            noise = _lib.nrx_gen_noise()
            noise.no_slot = no.data_ptr()
        d = self.p.desc(batch, 0.0 if noise is not None else no, slot_offset)
        o = _lib.nrx_gen_out()
        o.y, o.h_hat, o.h, o.active = ptr(sb.y), ptr(sb.h_hat), ptr(sb.h), ptr(sb.active)
        o.mcs_mask, o.mcs, o.bits, o.bits_stride = ptr(sb.mcs_mask), ptr(sb.mcs), ptr(sb.bits), self.p.bits_max
        o.y_real, o.y_imag = ptr(sb.y_real), ptr(sb.y_imag)
        o.h_ls_real, o.h_ls_imag = ptr(sb.h_ls_real), ptr(sb.h_ls_imag)
        if self._cfo is not None:
            self._cfo.eps_out = ptr(sb.cfo_eps)
        if self._dmrs is not None:
            self._dmrs.pilots_out = ptr(sb.pilots)
        if self._cir is not None and self._cir.select == SELECT["index"]:
            if cir_index is None:
                raise ValueError("select='index' needs cir_index")
            require("cir_index", cir_index, (batch, self.p.num_tx), torch.int32, sb.y.device)
            self._cir.index = cir_index.data_ptr()
        if self._td is not None:
            self._td.x_out = ptr(sb.x_td)
        if self._tc is not None:
            self._tc.r_out = ptr(sb.r_tc)
        # one entry point: the older nrx_generate_slots* are this call with NULL for the blocks they lack.
        # A dataset is the channel, so chan stays NULL with it (GenParams refuses the two together).
        blocks = (ref(d), ref(self._chan), ref(self._cfo), ref(self._dmrs), ref(self._cir), ref(self._td), ref(self._tc))
        run = (ref(o), ws.data_ptr(), ws.numel(), stream_of(sb.y, stream))
        if noise is None:
            _lib.check(self._lib.nrx_generate_slots_tc(*blocks, *run))
        else:
            _lib.check(self._lib.nrx_generate_slots_no(*blocks, ref(noise), *run))
        return sb

    def export_taps(self, batch: int, slot_offset: int = 0, stream=None) -> CIRDataset:
        """The built-in channel of slots ``slot_offset .. slot_offset + batch - 1`` as a device ``CIRDataset``
        (``nrx_generate_taps``): ``E = batch * U`` examples of ``num_taps`` paths and 14 time steps, example
        ``b * U + u``, taps and delays rounded once to float32.  Replaying it with ``select="index"``,
        ``f_offset="zero"`` and no normalisation gives this generator's channel again."""
        torch = _torch()
        if self._cir is not None:
            raise ValueError("export_taps exports the built-in channel; this generator replays a dataset")
        p, dev = self.p, f"cuda:{self.device}"
        E = batch * p.num_tx
        a = torch.empty((E, p.num_rx_ant, p.num_taps, NUM_SYMBOLS), dtype=torch.complex64, device=dev)
        tau = torch.empty((E, p.num_taps), dtype=torch.float32, device=dev)
        d = p.desc(batch, 0.0, slot_offset)
        ws = self._ws.get(self._ws.size(self._lib.nrx_gen_workspace_size, ref(d)), dev)
        _lib.check(self._lib.nrx_generate_taps(ref(d), ref(self._chan), a.data_ptr(), tau.data_ptr(), ws.data_ptr(),
                                               ws.numel(), stream_of(a, stream)))
        return CIRDataset(a, tau)


def count_errors(llr, bits, active, mcs, mcs_bits: Sequence[int], dmrs_syms: Sequence[int], counts=None,
                 stream=None):
    """Accumulate per-user uncoded counters ``counts [U, 4]`` int64 (bit errors, bits,
    block errors, blocks) on the device (include/nrx.h nrx_count_errors).  ``llr`` is the
    engine output ``[H, B, U, F, T, bits_stride]``; head = MCS index if H > 1."""
    torch = _torch()
    lib = _lib.load()
    H, B, U, F, T, bs = llr.shape
    if counts is None:
        counts = torch.zeros((U, 4), dtype=torch.int64, device=llr.device)
    if tuple(bits.shape) != (B, U, F, T, bs):
        raise ValueError(f"bits must be {(B, U, F, T, bs)}, got {tuple(bits.shape)}")
    c = _lib.nrx_count_io()
    fill_grid(c, B, U, F, T)
    fill_mcs(c, mcs_bits, dmrs_syms, bits_stride=bs, num_heads=H)
    c.llr, c.bits, c.active, c.counts, c.mcs = ptr(llr), ptr(bits), ptr(active), ptr(counts), ptr(mcs)
    _lib.check(lib.nrx_count_errors(ref(c), stream_of(llr, stream)))
    return counts
