"""Monte-Carlo evaluation of the neural receiver, all on the GPU.

The counterpart of the reference's ``scripts/evaluate.py`` NRX leg (evaluate.py:154-207:
``E2E_Model`` + ``load_weights`` + ``num_it = num_nrx_iter_eval`` + Sionna ``sim_ber``),
with the pieces that exist here: the GPU slot generator (``generator.SlotGenerator``),
the CGNN engine, the GPU error counters, and -- across ranks -- one RCCL
``all_reduce(SUM)`` of the int64 counters every ``sync_every`` Monte-Carlo iterations
(the analogue of ``sim_ber(distribute="all")``, evaluate.py:61).  Between those
reductions nothing leaves the device: the counters accumulate in HBM and the host runs
ahead, so a sharded run pays one collective + one host sync per window, not per batch.  The counts of a
``SimResult`` are uncoded: BER of hard decisions on the LLRs and the fraction of (slot, user) grids with any
bit error.  With ``coded`` (CLI: ``-ldpc``) every batch is also decoded by the GPU QC-LDPC decoder (``ldpc.py``)
and every system gains a coded BER / BLER column on the same slots.

sim_ber semantics kept: per Eb/N0 point iterate until ``max_mc_iter`` or until
``num_target_block_errors`` block errors (tested at each reduction, so a point may run
up to ``sync_every - 1`` batches past the target); ``early_stop`` ends the sweep at the first
point without errors; ``target_bler`` ends it once the BLER falls below the target.

    python -m neural_rx_amd.evaluate -config_name nrx_rt -num_tx_eval 2 \
        -ebno_db 0 2 4 6 8 -batch_size 128 -max_mc_iter 50

``-cfo_hz`` / ``-cfo_ppm`` add a per-user carrier frequency offset at the transmitter (the reference's
``cfo_offset_ppm_eval``); ``-cfo_comp`` runs every system behind the DMRS-based compensation of
``cfo.py``.  One stated departure: under a CFO the generator runs with ``h_with_phase``, so the
perfect-CSI systems and the NMSE see the diagonal of the effective channel; the reference hands its
perfect-CSI baselines the un-rotated channel, with which they collapse.

``-td_fft_size N`` puts the time-domain transmit stage of ``GenParams.td`` in front of the channel:
``-timing_offset`` (a late arrival per user) and ``-pa_ibo_db`` (a Rapp power amplifier) act on its samples, and
the generator runs with ``h_with_delay`` for the same reason.

``-tc_fft_size N`` replaces the per-RE channel product by the time-domain channel of ``GenParams.tc``: OFDM
modulation, per-sample Doppler and sinc delay taps (``-tc_l_min``, ``-tc_l_max``) on the samples, demodulation
with ``-tc_timing_advance``.  ``-max_doppler_hz`` and ``-max_delay_s`` set the spreads of the built-in channel
(inside a symbol a high Doppler is inter-carrier, a delay beyond ``-tc_cp`` inter-symbol interference); the
perfect-CSI systems and the NMSE see the ISI-free diagonal of the effective channel.

``-dmrs_cover`` gives the ``-num_tx_eval`` users orthogonal cover-coded DMRS ports (``ls.DMRSPorts``):
``h_hat`` is then the despreading LS estimate and users of one CDM group no longer collide on their
pilots; ``-dmrs_symbols 2 3 10 11`` supplies the symbol pairs that more than four ports need.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import time
from typing import List, Optional, Sequence

import numpy as np

from .config import get_config
from .generator import (SCENARIOS, GenParams, SlotGenerator, TimeChannelParams, TimeDomain, count_errors, ebno_to_no,
                        rx_correlation, scenario)
from .baseline import BaselineReceiver
from .chest import COV_SLOT_OFFSET, EstimatorBaselineReceiver, estimate_covariance
from .cfo import CFOCompensator
from .kbest import KBestBaselineReceiver
from .ls import DMRSPorts
from .receiver import CGNNEngine, compute_pe, spec_for


@dataclasses.dataclass
class SimResult:
    ebno_db: List[float]
    ber: List[float]
    bler: List[float]
    counts: List[List[int]]          # per point [bit_errors, bits, block_errors, blocks]
    mc_iters: List[int]
    seconds: float
    slots: int

    def as_dict(self):
        return dataclasses.asdict(self)


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


def _mc_loop(step, check, gen: SlotGenerator, ebno_dbs: Sequence[float], batch_size: int, max_mc_iter: int,
             num_target_block_errors: int, target_bler: Optional[float], early_stop: bool, verbose: bool,
             sync_every: int, label: Optional[str] = None, soft: Optional[list] = None, soft_h=None,
             soft_scales: Optional[Sequence[float]] = None, coded: Optional[list] = None,
             coded_spec=None) -> SimResult:
    """The Monte-Carlo loop shared by every system: ``step(sb, no) -> llr`` turns a generated batch
    into LLRs in the engine's layout, ``check()`` runs before every counter reduction.  Slot
    offsets, reductions and stopping rules do not depend on the system, so point k, iteration i
    is the same slot for every receiver and their curves are paired.

    ``soft``: a list that gains one ``softmetrics.SoftResult`` per Eb/N0 point -- the LLR statistics of
    every batch and, when ``soft_h() -> h_est`` returns the channel estimate of the batch just
    processed, its squared error against ``sb.h`` -- accumulated on the device and reduced over ranks
    at the same windows as the counters.  Without it the loop does what it did before.

    ``coded``: a list that gains one ``ldpc.CodedResult`` per Eb/N0 point -- the LLRs of every batch,
    descrambled by the sent bits, decoded towards the all-zero word with ``coded_spec``
    (``ldpc.DecoderSpec``) and counted on the device, reduced at the same windows.  ``no`` stays the one
    of ``ebno_to_no``: it is not re-adjusted by the code's rate.  The stopping rules keep looking at the
    uncoded counters, so the ``SimResult`` is the one of a call without ``coded``."""
    import torch
    if soft is not None:
        from .softmetrics import DEFAULT_SCALES, SoftAccumulator
    dist = _dist()
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
    # gloo (CPU tests, or ranks sharing one device) reduces host tensors; nccl = RCCL
    host_reduce = dist is not None and dist.get_backend() != "nccl"
    sync_every = max(1, int(sync_every))
    p = gen.p
    dev = torch.device(f"cuda:{gen.device}")
    res = SimResult([], [], [], [], [], 0.0, 0)
    cacc = None
    if coded is not None:
        from .ldpc import CodedAccumulator, DecoderSpec
        cacc = CodedAccumulator(coded_spec or DecoderSpec(), p.num_tx, p.mcs_bits,
                                p.num_subcarriers * (14 - len(p.dmrs_symbols)), device=gen.device)
    t0 = time.perf_counter()
    point_seed = 0
    for ebno in ebno_dbs:
        no = ebno_to_no(float(ebno), len(p.dmrs_symbols))
        counts = torch.zeros((p.num_tx, 4), dtype=torch.int64, device=dev)
        total = np.zeros(4, np.int64)
        acc = None
        if soft is not None:
            acc = SoftAccumulator(p.num_tx, p.mcs_bits, soft_scales or DEFAULT_SCALES, device=gen.device)
        if cacc is not None:
            cacc.reset()
        it = 0
        while it < max_mc_iter:
            off = ((point_seed * max_mc_iter + it) * world + rank) * batch_size
            sb = gen(batch_size, no, slot_offset=off)
            llr = step(sb, no)
            count_errors(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols, counts=counts)
            if acc is not None:
                acc.add_llr(llr, sb.bits, sb.active, sb.mcs, p.dmrs_symbols)
                h_est = soft_h() if soft_h is not None else None
                if h_est is not None:
                    acc.add_channel(h_est, sb.h, sb.active)
            if cacc is not None:
                cacc.add(llr, sb.bits, sb.active, sb.mcs, p.dmrs_symbols)
            it += 1
            if it % sync_every and it < max_mc_iter:
                continue
            check()
            tot = counts.sum(0)
            if host_reduce:
                tot = tot.cpu()
            if dist:
                dist.all_reduce(tot)
            total = tot.cpu().numpy()
            if acc is not None:
                acc.reduce(dist)
            if cacc is not None:
                cacc.reduce(dist)
            if total[2] >= num_target_block_errors:
                break
        ber = total[0] / total[1] if total[1] else float("nan")
        bler = total[2] / total[3] if total[3] else float("nan")
        res.ebno_db.append(float(ebno))
        res.ber.append(float(ber))
        res.bler.append(float(bler))
        res.counts.append([int(v) for v in total])
        res.mc_iters.append(it)
        res.slots += it * batch_size * world
        soft_txt = ""
        if acc is not None:
            sr = acc.result()
            soft.append(sr)
            soft_txt = "  " + soft_line(sr)
        if cacc is not None:
            cr = cacc.result()
            coded.append(cr)
            soft_txt += f"  coded[{cr.code} z{cr.z} x{cr.cw_per_block}] BER {cr.ber:.4e} BLER {cr.bler:.4e} it {cr.mean_iters:.2f}"
        if verbose and rank == 0:
            print(f"{label + '  ' if label else ''}EbNo {ebno:6.2f} dB  BER {ber:.4e}  BLER(uncoded) {bler:.4e}  "
                  f"bit errors {total[0]}  blocks {total[3]}  iters {it}{soft_txt}", flush=True)
        point_seed += 1
        if early_stop and total[0] == 0:
            break
        if target_bler is not None and bler < target_bler:
            break
    torch.cuda.synchronize(dev)
    res.seconds = time.perf_counter() - t0
    return res


class CfoStats:
    """Per noise level, the squared error of the DMRS-based CFO estimate against the generator's
    ``cfo_eps`` over the active (slot, user) pairs of this rank, accumulated on the device."""

    def __init__(self, comp: CFOCompensator):
        self.comp = comp
        self.acc = {}

    def add(self, sb, no: float) -> None:
        import torch
        err = (self.comp.estimate(sb) - sb.cfo_eps) * (sb.active > 0)
        v = torch.stack([(err * err).sum(), (sb.active > 0).sum().to(torch.float64)])
        self.acc[no] = self.acc[no] + v if no in self.acc else v

    def rms(self, no: float) -> Optional[float]:
        if no not in self.acc:
            return None
        s, n = self.acc[no].tolist()
        return float(np.sqrt(s / n)) if n else None


class CompensatedReceiver:
    """A baseline that reads ``sb.h_hat`` (``baseline.BaselineReceiver``) behind
    ``CFOCompensator.apply_nn``; the perfect-CSI systems pass through."""

    def __init__(self, receiver, comp: CFOCompensator):
        self.receiver, self.comp = receiver, comp
        self.perfect_csi = receiver.perfect_csi

    contaminated = property(lambda self: self.receiver.contaminated)
    last_h = property(lambda self: self.receiver.last_h)

    def __call__(self, sb, no, out=None, stream=None):
        if not self.perfect_csi:
            sb = self.comp.apply_nn(sb, stream=stream)
        return self.receiver(sb, no, out=out, stream=stream)


def soft_line(sr) -> str:
    """``BMI .. GMI .. (x scale) NMSE ..`` of a ``SoftResult``, one BMI / GMI per MCS"""
    f = lambda v: "-" if v is None or v != v else f"{v:.4f}"  # noqa: E731
    txt = "BMI " + "/".join(f(v) for v in sr.bmi) + "  GMI " + "/".join(
        f"{f(g)} (x{s:g})" if s == s else f(g) for g, s in zip(sr.gmi, sr.gmi_scale))
    txt += "  NMSE " + ("-" if sr.nmse is None else f"{sr.nmse:.4e}")
    if sr.nonfinite:
        txt += f"  non-finite LLRs {sr.nonfinite}"
    return txt


def sim_ber(engine: CGNNEngine, gen: SlotGenerator, ebno_dbs: Sequence[float], batch_size: int,
            max_mc_iter: int = 100, num_target_block_errors: int = 100, target_bler: Optional[float] = None,
            early_stop: bool = True, num_it: Optional[int] = None, precision: str = "f16",
            verbose: bool = False, sync_every: int = 8, soft: Optional[list] = None,
            soft_scales: Optional[Sequence[float]] = None, coded: Optional[list] = None,
            coded_spec=None) -> SimResult:
    """Sionna ``sim_ber`` loop on the GPU (this rank's shard of every Monte-Carlo batch:
    global slot ``(it * world + rank) * batch_size + b``).  The counters are reduced
    over ranks (and copied to the host) every ``sync_every`` batches and at the end of a
    point; every rank runs the same number of batches, so the collectives pair up.

    ``soft``: a list that gains one ``softmetrics.SoftResult`` per Eb/N0 point (BMI / GMI of the LLRs
    at ``soft_scales``, NMSE of the refined estimate ``h_ref``).  The forward then also runs the ChEst
    readout, and the generator needs ``want_h=True`` for the true channel.  The returned
    ``SimResult`` is the one of a call without ``soft``.

    ``coded``: a list that gains one ``ldpc.CodedResult`` per Eb/N0 point (coded BER / BLER, mean decoder
    iterations, code name, rate, N, C), decoded with ``coded_spec`` (``ldpc.DecoderSpec``; default r12, 20
    boxplus iterations).  ``no`` is not re-adjusted by the code's rate.  The ``SimResult`` is unchanged."""
    return _sim_ber_nrx(engine, gen, ebno_dbs, batch_size, max_mc_iter, num_target_block_errors, target_bler,
                        early_stop, num_it, precision, verbose, sync_every, None, soft, soft_scales, coded, coded_spec)


def _sim_ber_nrx(engine, gen, ebno_dbs, batch_size, max_mc_iter, num_target_block_errors, target_bler,
                 early_stop, num_it, precision, verbose, sync_every, label, soft=None, soft_scales=None,
                 coded=None, coded_spec=None, cfo=None, cfo_stats=None) -> SimResult:
    """sim_ber; ``label`` prefixes the verbose lines (the CLI's runs with baselines); ``cfo`` (a
    ``CFOCompensator``): the forward reads the compensated ``h_hat``; ``cfo_stats`` (``CfoStats``)
    gains every batch"""
    import torch
    p = gen.p
    dev = torch.device(f"cuda:{gen.device}")
    want_h = soft is not None
    if want_h and not gen.want_h:
        raise ValueError("the NMSE of the soft metrics needs the true channel: SlotGenerator(want_h=True)")
    pe = torch.from_numpy(compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)).to(dev)
    spec = engine.spec
    llr_out = engine.alloc_outputs(batch_size, p.num_tx, p.num_subcarriers, want_h=want_h)
    last = {}

    def step(sb, no):
        if cfo_stats is not None:
            cfo_stats.add(sb, no)
        if cfo is not None:
            sb = cfo.apply_nn(sb)
        mcs_mask = sb.mcs_mask if spec.num_mcs > 1 else None
        llr, last["h"] = engine.forward(sb.y, pe, sb.h_hat, sb.active, mcs_mask=mcs_mask, num_it=num_it,
                                        precision=precision, out=llr_out, want_h=want_h)
        return llr

    # engine.check: the one-launch forward's error word -- a timed-out or incomplete forward raises
    # at the reduction instead of entering the counts (include/nrx.h nrx_fused_status)
    return _mc_loop(step, engine.check, gen, ebno_dbs, batch_size, max_mc_iter, num_target_block_errors,
                    target_bler, early_stop, verbose, sync_every, label, soft, lambda: last["h"], soft_scales,
                    coded, coded_spec)


def sim_ber_baseline(receiver, gen: SlotGenerator, ebno_dbs: Sequence[float], batch_size: int,
                     max_mc_iter: int = 100, num_target_block_errors: int = 100,
                     target_bler: Optional[float] = None, early_stop: bool = True, verbose: bool = False,
                     sync_every: int = 8, label: Optional[str] = None, soft: Optional[list] = None,
                     soft_scales: Optional[Sequence[float]] = None, coded: Optional[list] = None,
                     coded_spec=None) -> SimResult:
    """``sim_ber`` with a classical baseline (``baseline.BaselineReceiver``,
    ``chest.EstimatorBaselineReceiver``, ``kbest.KBestBaselineReceiver``) in place of the engine:
    the same loop on the same slots (``_mc_loop``), so a baseline curve and the NRX curve of one
    generator are paired.  The perfect-CSI systems need ``SlotGenerator(want_h=True)``.

    ``soft``: as in ``sim_ber``; the NMSE is the one of the estimate the receiver detected with
    (``receiver.last_h``: ``sb.h_hat`` for the lsnn systems, the estimator's output for lslin / lmmse)
    and None for the perfect-CSI systems.  With an estimate to score, the generator needs
    ``want_h=True``.

    ``coded`` / ``coded_spec``: as in ``sim_ber``."""
    if receiver.perfect_csi and not gen.want_h:
        raise ValueError("a perfect-CSI baseline needs SlotGenerator(want_h=True)")
    soft_h = None
    if soft is not None and not receiver.perfect_csi:
        if not gen.want_h:
            raise ValueError("the NMSE of the soft metrics needs the true channel: SlotGenerator(want_h=True)")
        soft_h = lambda: receiver.last_h  # noqa: E731
    return _mc_loop(receiver, lambda: None, gen, ebno_dbs, batch_size, max_mc_iter, num_target_block_errors,
                    target_bler, early_stop, verbose, sync_every, label, soft, soft_h, soft_scales, coded, coded_spec)


def soft_dict(points, ebno_dbs: Sequence[float], code_rate: Optional[float] = None) -> dict:
    """The CLI's ``"soft"`` entry of one system: its ``SoftResult`` per Eb/N0 point and, with a code
    rate, the Eb/N0 at which the BMI and the GMI of each MCS reach it (``softmetrics.ebno_at_rate``;
    None where they do not)."""
    from .softmetrics import ebno_at_rate
    d = {"points": [sr.as_dict() for sr in points]}
    if code_rate is not None:
        d["code_rate"] = code_rate
        num_mcs = len(points[0].bmi) if points else 0
        d["ebno_at_rate"] = {
            key: [ebno_at_rate([(e, getattr(sr, key)[m]) for e, sr in zip(ebno_dbs, points)], code_rate)
                  for m in range(num_mcs)] for key in ("bmi", "gmi")}
    return d


def coded_dict(points) -> dict:
    """The CLI's ``"coded"`` entry of one system: its ``ldpc.CodedResult`` per Eb/N0 point"""
    return {"points": [cr.as_dict() for cr in points],
            "note": "no is the one of ebno_to_no, not re-adjusted by the code's rate; the project's own QC code"}


def baseline_note(name: str, receiver) -> Optional[str]:
    """The line the CLI prints beside a baseline curve that is not meaningful (baseline.py: LS
    estimates with two active ports on one CDM group), or None."""
    if not receiver.contaminated:
        return None
    return (f"{name}: note: active ports can share a CDM group and the generator applies no cover code, "
            "so h_hat is pilot-contaminated and this curve is not a meaningful baseline")


def add_arguments(ap, generator_only=False):
    """The options of the command line.  ``generator_only``: just those that choose the configuration and the
    generated slots -- what ``train.py`` shares with the evaluation (``generator_params`` reads them)."""
    ev = (lambda *args, **kw: None) if generator_only else ap.add_argument   # the evaluation's own options
    ap.add_argument("-config_name", default="nrx_rt")
    ap.add_argument("-num_tx_eval", type=int, default=None, help="active DMRS ports per slot")
    ap.add_argument("-num_prbs", type=int, default=None)
    ev("-ebno_db", type=float, nargs="+", default=None)
    ap.add_argument("-batch_size", type=int, default=128)
    ev("-max_mc_iter", type=int, default=100)
    ev("-num_target_block_errors", type=int, default=500)
    ev("-target_bler", type=float, default=None)
    ap.add_argument("-var_mcs", action="store_true", help="draw the MCS of every (slot, user)")
    ev("-precision", default="f16")
    ap.add_argument("-seed", type=int, default=1234)
    ev("-sync_every", type=int, default=8, help="MC batches per counter all-reduce")
    ap.add_argument("-gpu", type=int, default=None)
    ev("-out", default=None, help="write the result JSON here")
    ev("-weights", default=None, metavar="FILE.npz",
       help="score this weight file (weights.save, train.py -out) in place of the config's shipped weights")
    ev("-baselines", nargs="*", default=[],
       choices=["lsnn_lmmse", "lslin_lmmse", "lmmse_lmmse", "perf_csi_lmmse", "lmmse_kbest", "perf_csi_kbest"],
       help="classical baselines run on the same slots (baseline.BaselineReceiver, "
            "chest.EstimatorBaselineReceiver, kbest.KBestBaselineReceiver); the JSON gains "
            "\"baselines\": {name: result}")
    ev("-kbest_k", type=int, default=64, help="survivors per level of the K-best baselines (1..64)")
    ev("-num_cov_slots", type=int, default=2048,
       help="slots the covariance of lmmse_lmmse / lmmse_kbest is estimated from (drawn at slot offset 2^40, "
            "disjoint from every Monte-Carlo slot)")
    ev("-soft_metrics", action="store_true",
       help="also accumulate the soft-output metrics (softmetrics.py): BMI / GMI of every system's "
            "LLRs and the NMSE of its channel estimate; the JSON gains \"soft\" (per point) next to "
            "every result")
    ev("-llr_scales", type=float, nargs="+", default=None,
       help="LLR scale factors the GMI is searched over (1..16 positive numbers)")
    ev("-code_rate", type=float, default=None,
       help="with -soft_metrics: report the Eb/N0 at which BMI and GMI reach this rate")
    ev("-ldpc", default=None, choices=["r13", "r12", "r23", "r34"],
       help="also decode every batch with the GPU QC-LDPC decoder (ldpc.py; the project's own regular "
            "code of that rate, sized to the slot) and report coded BER / BLER for every system; the "
            "JSON gains \"coded\" next to every result")
    ev("-ldpc_iter", type=int, default=20, help="decoder iterations (1..100), with early stop")
    ev("-ldpc_cn", default="boxplus", choices=["boxplus", "minsum"], help="check-node update")
    ap.add_argument("-cir_file", default=None, metavar="PATH",
                    help="-channel dataset: the .npz of channel impulse responses to replay (cir.CIRDataset: 'a' "
                         "complex64 [E, A, L, 1 | 14], 'tau' float32 [E, L] in seconds)")
    ap.add_argument("-cir_select", default="random", choices=["random", "trajectory"],
                    help="example of a (slot, user): any, or user u on the examples that are u modulo the users")
    ap.add_argument("-cir_no_norm", action="store_true", help="keep the dataset's energy (default: unit mean energy "
                                                              "per (slot, user) over the grid)")
    ap.add_argument("-cir_f_zero", action="store_true", help="subcarrier 0 at frequency 0 (default: centred grid)")
    ap.add_argument("-channel", default="iid", choices=["iid", "dataset"] + list(SCENARIOS),
                    help="iid: one delay / Doppler profile for every user and uncorrelated receive antennas; "
                         "double_tdl_low / double_tdl_high: the two-user profiles of the reference's evaluation "
                         "channel with gNB antenna correlation alpha = 0 / 0.9 (generator.scenario; needs a "
                         "two-port config)")
    ap.add_argument("-rx_corr", type=float, default=None, metavar="ALPHA",
                    help="receive-antenna correlation rx_correlation(A, ALPHA), replacing the channel's own")
    ev("-chest_2d", action="store_true",
       help="on a correlated channel lmmse_lmmse uses the spatial covariance (nrx_chest_lmmse3); this "
            "keeps the 2-D filter that ignores it, so that both can be tabulated")
    ap.add_argument("-cfo_hz", type=float, default=None, metavar="HZ",
                    help="per-user carrier frequency offset at the transmitter, drawn uniformly in +-HZ per "
                         "(slot, user) (GenParams.cfo_hz); the generator then runs with h_with_phase")
    ap.add_argument("-cfo_ppm", type=float, default=None, metavar="PPM",
                    help="the same as a fraction of the carrier: HZ = carrier_frequency_hz / 1e6 * PPM")
    ap.add_argument("-carrier_frequency_hz", type=float, default=2.14e9)
    ap.add_argument("-cfo_constant", action="store_true", help="every user has exactly the offset, not a draw")
    ev("-cfo_comp", action="store_true",
       help="DMRS-based CFO estimation and compensation (cfo.py) in front of every system: the NRX and "
            "lsnn_lmmse read the compensated h_hat, the estimators run between a de-rotation and a "
            "re-rotation")
    ap.add_argument("-dmrs_cover", action="store_true",
                    help="cover-coded DMRS ports (ls.DMRSPorts.for_config) for -num_tx_eval users, all active: CDM "
                         "group x frequency cover x time cover, despread by the LS estimator (nrx_ls_estimate); more "
                         "than 4 users need DMRS symbols in pairs (-dmrs_symbols 2 3 10 11)")
    ap.add_argument("-dmrs_symbols", type=int, nargs="+", default=None, metavar="T",
                    help="DMRS symbols in place of the config's, ascending, at most 4; the positional encoding, the "
                         "data REs, the pilot overhead of Eb/N0 and the LDPC code size follow")
    ap.add_argument("-td_fft_size", type=int, default=None, metavar="N",
                    help="a time-domain transmit stage between the grid and the channel (GenParams.td): OFDM "
                         "modulation at FFT size N (a power of two, 64..4096, at least the grid), the impairments "
                         "below on the samples, demodulation; the generator then runs with h_with_delay")
    ap.add_argument("-td_cp", type=int, default=None, metavar="L", help="cyclic prefix in samples (default 9 N / 128)")
    ap.add_argument("-pa_ibo_db", type=float, default=None, metavar="X",
                    help="Rapp power amplifier at this input back-off over the nominal sample power (needs -td_fft_size)")
    ap.add_argument("-pa_smoothness", type=float, default=2.0, metavar="P", help="the Rapp curve's p")
    ap.add_argument("-timing_offset", type=int, nargs="+", default=None, metavar="D",
                    help="samples by which a user's signal arrives late, one value or one per user (needs "
                         "-td_fft_size); beyond the cyclic prefix it is inter-symbol interference")
    ap.add_argument("-tc_fft_size", type=int, default=None, metavar="N",
                    help="the time-domain channel in place of the per-RE product (GenParams.tc): OFDM modulation at "
                         "FFT size N (a power of two, 64..4096, at least the grid), per-sample Doppler and sinc "
                         "delay taps on the samples, demodulation; h is the ISI-free diagonal of the effective channel")
    ap.add_argument("-tc_cp", type=int, default=None, metavar="L", help="cyclic prefix in samples (default 9 N / 128)")
    ap.add_argument("-tc_l_min", type=int, default=-6, metavar="L", help="first tap of the truncated sinc, <= 0")
    ap.add_argument("-tc_l_max", type=int, default=None, metavar="L",
                    help="last tap (default: the longest delay in samples, rounded up, + 6)")
    ap.add_argument("-tc_timing_advance", type=int, default=0, metavar="D",
                    help="the receive windows start D samples early, 0..cyclic prefix")
    ap.add_argument("-max_doppler_hz", type=float, default=None, metavar="HZ",
                    help="maximum Doppler shift of the built-in channel (GenParams.max_doppler_hz; -channel iid)")
    ap.add_argument("-max_delay_s", type=float, default=None, metavar="S",
                    help="maximum path delay of the built-in channel (GenParams.max_delay_s; -channel iid)")


def check_arguments(ap, a):
    """the refusals among the generator's options, which come before the first import of torch"""
    if a.tc_fft_size is None and (a.tc_cp is not None or a.tc_l_max is not None or a.tc_timing_advance or a.tc_l_min != -6):
        ap.error("-tc_cp, -tc_l_min, -tc_l_max and -tc_timing_advance belong to the time-domain channel: give -tc_fft_size")
    if a.tc_fft_size is not None and (a.td_fft_size is not None or a.cfo_hz is not None or a.cfo_ppm is not None
                                      or a.channel == "dataset"):
        ap.error("-tc_fft_size with -td_fft_size, a CFO or -channel dataset: a run takes one sample-domain stage")
    if a.channel != "iid" and (a.max_doppler_hz is not None or a.max_delay_s is not None):
        ap.error("-max_doppler_hz and -max_delay_s set the spreads of -channel iid; the other channels bring their own")
    if a.td_fft_size is None and (a.pa_ibo_db is not None or a.timing_offset is not None or a.td_cp is not None):
        ap.error("-pa_ibo_db, -timing_offset and -td_cp act on the samples of the time-domain stage: give -td_fft_size")
    if a.td_fft_size is not None and (a.cfo_hz is not None or a.cfo_ppm is not None):
        ap.error("-td_fft_size and a CFO are two transmit-side stages: give one")
    if a.cfo_hz is not None and a.cfo_ppm is not None:
        ap.error("-cfo_hz and -cfo_ppm are two ways to say the same thing: give one")
    if (a.channel == "dataset") != (a.cir_file is not None):
        ap.error("-channel dataset and -cir_file PATH go together")
    if a.channel == "dataset" and a.rx_corr is not None:
        ap.error("-rx_corr does not apply to -channel dataset: the dataset brings its own antenna structure")


def generator_params(a, cfg):
    """``(GenParams, ports, cfo_hz)`` of the parsed options ``a`` (``add_arguments``) for config ``cfg``"""
    u = (a.num_tx_eval or cfg.max_num_tx) if a.dmrs_cover else cfg.max_num_tx
    params = GenParams.from_config(cfg, num_tx=u, num_prbs=a.num_prbs, var_mcs=a.var_mcs, seed=a.seed)
    if a.dmrs_symbols is not None:
        params = dataclasses.replace(params, dmrs_symbols=tuple(a.dmrs_symbols))
    if a.dmrs_cover:
        params = dataclasses.replace(params, dmrs=DMRSPorts.for_config(cfg, u))
    params.num_active = a.num_tx_eval or u
    if a.max_doppler_hz is not None:
        params = dataclasses.replace(params, max_doppler_hz=a.max_doppler_hz)
    if a.max_delay_s is not None:
        params = dataclasses.replace(params, max_delay_s=a.max_delay_s)
    if a.channel == "dataset":
        from .cir import CIRChannel, CIRDataset
        params = dataclasses.replace(params, cir=CIRChannel(
            CIRDataset.load(a.cir_file), select=a.cir_select, normalize=not a.cir_no_norm,
            f_offset="zero" if a.cir_f_zero else "centered"))
    elif a.channel != "iid":
        params = scenario(a.channel, params)
    if a.rx_corr is not None:
        params = dataclasses.replace(params, rx_corr=rx_correlation(params.num_rx_ant, a.rx_corr))
    cfo_hz = a.cfo_hz if a.cfo_hz is not None else \
        a.carrier_frequency_hz / 1e6 * a.cfo_ppm if a.cfo_ppm is not None else None
    if cfo_hz is not None:
        params = dataclasses.replace(params, cfo_hz=cfo_hz, cfo_constant=a.cfo_constant, h_with_phase=True)
    if a.td_fft_size is not None:
        delay = a.timing_offset if a.timing_offset is not None else [0]
        params = dataclasses.replace(params, td=TimeDomain(
            fft_size=a.td_fft_size, cp=a.td_cp, delay=delay[0] if len(delay) == 1 else tuple(delay),
            pa_ibo_db=a.pa_ibo_db, pa_smoothness=a.pa_smoothness, h_with_delay=True))
    if a.tc_fft_size is not None:
        params = dataclasses.replace(params, tc=TimeChannelParams(
            fft_size=a.tc_fft_size, cp=a.tc_cp, l_min=a.tc_l_min, l_max=a.tc_l_max,
            timing_advance=a.tc_timing_advance))
    return params, u, cfo_hz


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_arguments(ap, a)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    device = a.gpu if a.gpu is not None else local
    torch.cuda.set_device(device)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{device}"))
    cfg = get_config(a.config_name)
    spec = spec_for(cfg)
    from . import weights as W
    engine = CGNNEngine(spec, W.load_file(a.weights) if a.weights else W.load(cfg.label), device=device)
    params, u, cfo_hz = generator_params(a, cfg)
    # a correlated channel: the LMMSE estimator takes the spatial covariance unless -chest_2d keeps it out
    # (a replayed dataset counts as one: its antennas are as correlated as its geometry makes them)
    chest3 = (params.rx_corr is not None or params.cir is not None) and not a.chest_2d
    systems = {n: "baseline_" + n for n in a.baselines}
    needs_h = {"perf_csi_lmmse", "lmmse_lmmse", "perf_csi_kbest", "lmmse_kbest"}
    gen = SlotGenerator(params, device=device, want_h=bool(needs_h & set(systems)) or a.soft_metrics)
    ebno = a.ebno_db if a.ebno_db is not None else list(np.arange(-2.0, 8.0, 1.0))
    soft = {"nrx": []} if a.soft_metrics else {}
    coded = {"nrx": []} if a.ldpc else {}
    coded_spec = None
    if a.ldpc:
        from .ldpc import DecoderSpec
        coded_spec = DecoderSpec(code_name=a.ldpc, num_iter=a.ldpc_iter, cn_type=a.ldpc_cn)
    comp = CFOCompensator(params, device=device) if a.cfo_comp or cfo_hz is not None else None
    cfo_stats = CfoStats(comp) if cfo_hz is not None else None
    comp = comp if a.cfo_comp else None
    res = _sim_ber_nrx(engine, gen, ebno, a.batch_size, a.max_mc_iter, a.num_target_block_errors, a.target_bler,
                       True, cfg.num_nrx_iter_eval, a.precision, True, a.sync_every, "nrx" if systems else None,
                       soft.get("nrx"), a.llr_scales, coded.get("nrx"), coded_spec, comp, cfo_stats)
    base = {}
    cov = None
    if {"lmmse_lmmse", "lmmse_kbest"} & set(systems):
        # the counterpart of compute_cov_mat.py before evaluate (scripts/evaluate.py:159); every rank
        # estimates the same matrices from the same slots
        if a.num_cov_slots < 1 or COV_SLOT_OFFSET <= len(ebno) * a.max_mc_iter * world * a.batch_size:
            raise ValueError("-num_cov_slots must be >= 1 and the Monte-Carlo slots must end below 2^40")
        # behind the compensation the estimator sees de-rotated pilots: its covariance is the one of the
        # channel without the offset
        cov_gen = gen if comp is None or cfo_hz is None else \
            SlotGenerator(dataclasses.replace(params, cfo_hz=None), device=device, want_h=True)
        est = estimate_covariance(cov_gen, a.num_cov_slots, a.batch_size)
        cov = est.matrices()
        R_s = est.space() if chest3 else None
    for name, system in systems.items():
        if system in KBestBaselineReceiver.SYSTEMS:
            rx = KBestBaselineReceiver(system, params, device=device, k=a.kbest_k, cfo=comp)
            if cov is not None:
                rx.set_covariance(*cov)
        elif system in EstimatorBaselineReceiver.SYSTEMS:
            # the filter is designed again at every Eb/N0 point (ChannelEstimator.prepare)
            rx = EstimatorBaselineReceiver(system, params, device=device, cfo=comp)
            if cov is not None:
                rx.set_covariance(*cov, R_s=R_s)
        else:
            rx = BaselineReceiver(system, params, device=device)
            if comp is not None:
                rx = CompensatedReceiver(rx, comp)
        note = baseline_note(name, rx)
        if note and rank == 0:
            print(note, flush=True)
        if a.soft_metrics:
            soft[name] = []
        if a.ldpc:
            coded[name] = []
        base[name] = sim_ber_baseline(rx, gen, ebno, a.batch_size, a.max_mc_iter, a.num_target_block_errors,
                                      a.target_bler, verbose=True, sync_every=a.sync_every, label=name,
                                      soft=soft.get(name), soft_scales=a.llr_scales, coded=coded.get(name),
                                      coded_spec=coded_spec)
    d = None
    if rank == 0:
        d = res.as_dict()
        d.update(config=cfg.label, num_tx_eval=params.num_active, dmrs_symbols=list(params.dmrs_symbols),
                 world=world, slots_per_s=res.slots / res.seconds)
        if a.dmrs_cover:            # a run without it keeps the keys it always had
            d["dmrs_cover"] = dict(cdm_group=list(params.dmrs.cdm_group), focc=list(params.dmrs.focc),
                                   tocc=list(params.dmrs.tocc), block=params.dmrs.block)
        if params.correlated:       # the iid run keeps the keys it always had
            d.update(channel=a.channel, user_profiles=[list(x) for x in params.profiles()],
                     rx_corr=a.rx_corr if a.rx_corr is not None else SCENARIOS.get(a.channel),
                     chest="lmmse3" if chest3 else "lmmse")
        if params.cir is not None:
            ds = params.cir.dataset
            d.update(channel=a.channel, chest="lmmse3" if chest3 else "lmmse",
                     cir=dict(file=a.cir_file, select=a.cir_select, normalize=not a.cir_no_norm,
                              f_offset=params.cir.offset(params.num_subcarriers), num_examples=ds.num_examples,
                              num_paths=ds.num_paths, num_time_steps=ds.num_time_steps))
        if cfo_hz is not None or a.cfo_comp:       # a run without either keeps the keys it always had
            d["cfo"] = dict(cfo_hz=cfo_hz, cfo_ppm=a.cfo_ppm, carrier_frequency_hz=a.carrier_frequency_hz,
                            constant=a.cfo_constant, comp=a.cfo_comp, h_with_phase=cfo_hz is not None,
                            subcarrier_spacing=params.subcarrier_spacing)
            if cfo_stats is not None:
                # rms of eps_hat - eps (in subcarrier spacings) over this rank's active (slot, user) pairs
                d["cfo"]["eps_rms_error"] = [cfo_stats.rms(ebno_to_no(float(e), len(params.dmrs_symbols)))
                                             for e in res.ebno_db]
        if params.td is not None:                  # a run without the stage keeps the keys it always had
            d["td"] = dict(fft_size=params.td.fft_size, cp=params.td.cp_list(), delay=params.td.delay_per_port(u),
                           pa_ibo_db=params.td.pa_ibo_db, pa_smoothness=params.td.pa_smoothness, h_with_delay=True)
        if params.tc is not None:
            d["tc"] = dict(fft_size=params.tc.fft_size, cp=params.tc.cp_list(), l_min=params.tc.l_min,
                           l_max=params.tc.l_max, timing_advance=params.tc.timing_advance,
                           max_doppler_hz=params.max_doppler_hz, max_delay_s=params.max_delay_s)
        if base:
            d["baselines"] = {name: r.as_dict() for name, r in base.items()}
        for name, points in soft.items():
            sd = soft_dict(points, (res if name == "nrx" else base[name]).ebno_db, a.code_rate)
            if rank == 0 and a.code_rate is not None:
                print(f"{name}  Eb/N0 at rate {a.code_rate:g}: BMI {sd['ebno_at_rate']['bmi']}  "
                      f"GMI {sd['ebno_at_rate']['gmi']}", flush=True)
            (d if name == "nrx" else d["baselines"][name])["soft"] = sd
        for name, points in coded.items():
            (d if name == "nrx" else d["baselines"][name])["coded"] = coded_dict(points)
        if cov is not None:
            d["num_cov_slots"] = a.num_cov_slots
        print(json.dumps(d))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(d, f)
    if world > 1:
        dist.destroy_process_group()
    return d


if __name__ == "__main__":
    main()
