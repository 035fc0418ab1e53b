"""Which value test reaches which kernel instantiation of the baseline dispatchers.  A table, not a test;
tests/test_dispatch_cases.py keeps it complete against the launchers' source.

The classical kernels (detectors, channel estimators, LS estimator, LLR statistics, error counters, time-domain
channel, OFDM) pick their kernel on the host: a ``switch`` over a template parameter, a ``vec`` flag from the
alignment and the antenna count, or a chain of ``if (...) return launch<...>``.  For every such dispatcher this
module names the dispatched value and, per label, one test that runs the label's kernel and compares its output
with the numpy reference of its file.

    DISPATCH[launcher] = (source file under neural_rx_amd/csrc, what is dispatched on, [table per switch])

A table maps a label to a test: ``"case 5"`` / ``"default"`` of a ``switch``, or the instantiation a ``return``
of an if-chain launches.  Where the label's statement passes ``vec`` on, the kernel exists twice and the keys are
``("case 5", "vec")`` and ``("case 5", "scalar")``.  A test is ``T(module, function, **params)``: the params are
argument values of one row of the function's ``parametrize`` lists (none for a test that loops inside).  A label
the public entry point refuses before the launch names the CPU test that shows the refusal.

BRANCHES lists, in the same form, the host-side branches that are no label: pass counts, tile tails and block
shapes that a launcher derives from the shape.
"""
from __future__ import annotations

from typing import NamedTuple


class T(NamedTuple):
    module: str
    function: str
    params: dict

    @classmethod
    def of(cls, module: str, function: str, **params) -> "T":
        return cls("tests." + module, function, params)


_lm = lambda name: T.of("test_gpu_lmmse", "test_case", name=name)                        # noqa: E731
_lm_unaligned = T.of("test_gpu_lmmse", "test_unaligned_tensors_take_the_scalar_paths")   # C1, C6, C3, C2: U 2, 3, 4, 8
_kb = lambda name: T.of("test_gpu_kbest", "test_case", name=name)                        # noqa: E731
_kb_unaligned = T.of("test_gpu_kbest", "test_unaligned_tensors_take_the_scalar_paths")   # U 4, 1, 2, 3, 6, 7, 8
_ch = lambda name: T.of("test_gpu_chest", "test_estimator_against_the_oracle", name=name, kind="lmmse")  # noqa: E731
_ch_unaligned = T.of("test_gpu_chest", "test_unaligned_output_takes_the_scalar_path")    # K1, K3, K6, K7
_c3 = lambda name: T.of("test_gpu_chest3", "test_estimator_against_the_oracle", name=name)   # noqa: E731
_c3_unaligned = T.of("test_gpu_chest3", "test_unaligned_output_takes_the_scalar_path")   # K1, K3, K6
_ls = lambda F, A: T.of("test_gpu_ls", "test_estimator_matches_reference", F=F, A=A)     # noqa: E731
_sm = lambda name: T.of("test_gpu_softmetrics", "test_llr_stats_match_the_reference", name=name)   # noqa: E731
_cnt = lambda bs: T.of("test_gpu_synth", "test_error_counters_many_slots", bs=bs)        # noqa: E731
_tc = lambda A, Ls: T.of("test_gpu_timechan", "test_against_the_statement", A=A, Ls=Ls)  # noqa: E731
_tce = lambda A: T.of("test_gpu_timechan", "test_edges_of_the_kernel_shapes", A=A)       # noqa: E731
_ofdm = lambda N: T.of("test_gpu_ofdm", "test_modulate", N=N)                            # noqa: E731

DISPATCH = {
    "launch_lmmse": ("nrx_lmmse.hip", "num_tx (U); vec: A % 4 == 0 and 16-byte aligned y, h", [{
        ("case 1", "vec"): _lm("C13"), ("case 1", "scalar"): _lm("C4"),
        ("case 2", "vec"): _lm("C1"), ("case 2", "scalar"): _lm_unaligned,
        ("case 3", "vec"): _lm("C6"), ("case 3", "scalar"): _lm_unaligned,
        ("case 4", "vec"): _lm("C3"), ("case 4", "scalar"): _lm_unaligned,
        ("case 5", "vec"): _lm("C7"), ("case 5", "scalar"): _lm("C10"),
        ("case 6", "vec"): _lm("C8"), ("case 6", "scalar"): _lm("C11"),
        ("case 7", "vec"): _lm("C9"), ("case 7", "scalar"): _lm("C12"),
        ("case 8", "vec"): _lm("C2"), ("case 8", "scalar"): _lm_unaligned,
        "default": T.of("test_lmmse_ref", "test_argument_checks", kw=dict(num_tx=9)),
    }]),
    "launch_kbest": ("nrx_kbest.hip", "num_tx (U); vec: even A and 8-byte aligned y, h", [{
        ("case 1", "vec"): _kb("K1"), ("case 1", "scalar"): _kb_unaligned,
        ("case 2", "vec"): _kb("K4"), ("case 2", "scalar"): _kb_unaligned,
        ("case 3", "vec"): _kb("K2"), ("case 3", "scalar"): _kb_unaligned,
        ("case 4", "vec"): _kb("K3"), ("case 4", "scalar"): _kb_unaligned,
        ("case 5", "vec"): _kb("K7"), ("case 5", "scalar"): _kb("K10"),
        ("case 6", "vec"): _kb("K8"), ("case 6", "scalar"): _kb_unaligned,
        ("case 7", "vec"): _kb("K9"), ("case 7", "scalar"): _kb_unaligned,
        ("case 8", "vec"): _kb("K5"), ("case 8", "scalar"): _kb_unaligned,
        "default": T.of("test_kbest_ref", "test_argument_checks", kw=dict(num_tx=9)),
    }]),
    "launch_chest_lmmse": ("nrx_chest.hip", "num_dmrs_symbols (nd); vec: A % 4 == 0 and 16-byte aligned h_out", [{
        ("case 1", "vec"): _ch("K8"), ("case 1", "scalar"): _ch("K2"),
        ("case 2", "vec"): _ch("K1"), ("case 2", "scalar"): _ch("K5"),
        ("case 3", "vec"): _ch("K3"), ("case 3", "scalar"): _ch_unaligned,
        ("case 4", "vec"): _ch("K6"), ("case 4", "scalar"): _ch("K7"),
        "default": T.of("test_chest_ref", "test_chest_lmmse_argument_checks", kw=dict(num_dmrs_symbols=5)),
    }]),
    "launch_chest_lmmse3": ("nrx_chest.hip", "num_dmrs_symbols (nd); vec as launch_chest_lmmse (k_chest3_expand)", [{
        ("case 1", "vec"): _c3("K7"), ("case 1", "scalar"): _c3("K2"),
        ("case 2", "vec"): _c3("K1"), ("case 2", "scalar"): _c3("K4"),
        ("case 3", "vec"): _c3("K3"), ("case 3", "scalar"): _c3_unaligned,
        ("case 4", "vec"): _c3("K6"), ("case 4", "scalar"): _c3_unaligned,
        "default": T.of("test_chest3_ref", "test_chest3_argument_checks", kw=dict(num_dmrs_symbols=5)),
    }]),
    "launch_ls_estimate": ("nrx_ls.hip", "2 * num_rx_ant (A2C)", [{
        "case 4": _ls(8, 2), "case 8": _ls(24, 4), "case 16": _ls(24, 8), "case 32": _ls(24, 16),
        "default": _ls(24, 3),
    }]),
    "launch_llr_stats": ("nrx_softmetrics.hip", "bits_stride with the row alignment (BSC); num_mcs (MM)", [
        {"case 2": _sm("S5"), "case 4": _sm("S1"), "case 6": _sm("S2"), "case 8": _sm("S4"), "default": _sm("S6")},
        {"case 1": _sm("S1"), "case 2": _sm("S3"), "case 3": _sm("S2"), "case 4": _sm("S8"), "default": _sm("S7")},
    ]),
    "launch_count_errors": ("nrx_synth.hip", "bits_stride", [{
        "case 2": _cnt(2), "case 4": _cnt(4), "case 6": _cnt(6), "case 8": _cnt(8), "default": _cnt(5),
    }]),
    "launch_tc_args": ("nrx_timechan.hip", "num_rx_ant: A <= 4, <= 8, else", [{
        "launch_tc_k<4, 4>": _tce(4), "launch_tc_k<8, 2>": _tce(8), "launch_tc_k<16, 1>": _tce(16),
    }]),
    "launch_n": ("nrx_ofdm.hip", "fft_size: N <= 1024, 2048, else (butterflies per thread)", [{
        "launch_k<R, MOD, 1>": _ofdm(64), "launch_k<R, MOD, 2>": _ofdm(2048), "launch_k<R, MOD, 4>": _ofdm(4096),
    }]),
}

# host-side branches without a label: (launcher, branch) -> test
BRANCHES = {
    ("launch_lmmse", "VEC && U >= 7: two antennas per step, U = 7"): _lm("C9"),
    ("launch_lmmse", "U >= 7 with scalar loads"): _lm("C12"),
    ("launch_kbest", "search at 10, 12, 14 levels"): _kb("K9"),
    ("launch_kbest", "nd > kSearchGridMax: a wave takes a second resource element"): _kb("K11"),
    ("launch_ls_estimate", "ports_per_pass < U: two passes of 4 ports"): _ls(24, 16),
    ("launch_ls_estimate", "passes of 4 + 3 ports, two tiles, the second partial"): _ls(40, 16),
    ("launch_llr_stats", "B > kRedSlots and more records than a tile: the ordered pass repeats"): _sm("S9"),
    ("launch_tc_args", "NS = 16: 64 sinusoid rows per chunk, every chunk full (A = 16)"): _tce(16),
    ("launch_tc_args", "NS = 1, A = 1, L = 8"): _tce(1),
    ("launch_tc_args", "L = 1, U = 1"): _tce(4),
    ("launch_tc_args", "several tiles per row, the last partial"): _tc(5, 2500),
    ("launch_tc_rx", "k_tc_h FB = 3 with a two-subcarrier last block"):
        T.of("test_gpu_synth_tc", "test_channel_against_the_statement_at_other_block_shapes", A_=5, F_=50),
    ("launch_tc_rx", "k_tc_h FB = 1"):
        T.of("test_gpu_synth_tc", "test_channel_against_the_statement_at_other_block_shapes", A_=16, F_=48),
    ("launch_tc_rx", "k_tc_h FB = 2, F % FB == 0 at an odd block count"):
        T.of("test_gpu_synth_tc", "test_channel_against_the_statement_at_other_block_shapes", A_=8, F_=46),
    ("launch_tc_rx", "k_tc_h FB = 4"): T.of("test_gpu_synth_tc", "test_channel_against_the_statement", doppler=20e3),
}
