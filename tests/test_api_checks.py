"""Argument checks of the handle-free entry points that the per-feature test files leave untabulated
(nrx_count_errors, nrx_llr_demap, nrx_compute_pe, the generator, the rest of nrx_lmmse_detect and
nrx_cov_*), and the rules that differ between entry points on purpose.  Every check runs before the
first HIP call, so the status codes are checked here without a GPU: the pointers are non-null dummies
that are never dereferenced, and every case breaks one rule."""
import ctypes

import pytest

from neural_rx_amd import _lib

OK, INVALID_ARG, SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -6
PTR = 4096
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _set(io, kw):
    """mcs_bits1=3 sets io.mcs_bits[1]; the same for every other array field"""
    for k, v in kw.items():
        name = k.rstrip("0123456789")
        if name != k and not hasattr(io, k):
            getattr(io, name)[int(k[len(name):])] = v
        else:
            setattr(io, k, v)
    return io


def _grid(io, **extra):
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    for k, v in extra.items():
        setattr(io, k, v)
    return io


def _mcs(io):
    io.bits_stride, io.num_mcs = 6, 3
    io.mcs_bits[0], io.mcs_bits[1], io.mcs_bits[2] = 2, 4, 6
    io.dmrs_symbol_mask = (1 << 2) | (1 << 11)
    return io


def _count_io(**kw):
    io = _mcs(_grid(_lib.nrx_count_io(), num_heads=1))
    io.llr = io.bits = io.mcs = io.active = io.counts = PTR
    return _set(io, kw)


def _lmmse_io(**kw):
    io = _mcs(_grid(_lib.nrx_lmmse_io(), num_rx_ant=4))
    io.no, io.err_var = 0.1, 0.0
    io.y = io.h = io.active = io.mcs = io.llr = PTR
    return _set(io, kw)


def _kbest_io(**kw):
    io = _mcs(_grid(_lib.nrx_kbest_io(), num_rx_ant=4, k=8))
    io.no, io.err_var, io.llr_clip = 0.1, 0.0, 20.0
    io.y = io.h = io.active = io.mcs = io.llr = PTR
    return _set(io, kw)


def _cov_io(cls=None, **kw):
    io = _grid((cls or _lib.nrx_cov_io)(), num_rx_ant=4)
    io.h = io.acc = PTR
    return _set(io, kw)


def _nmse_io(**kw):
    io = _grid(_lib.nrx_nmse_io(), num_rx_ant=4, symbol_mask=0)
    io.h_est = io.h_true = io.active = io.err = io.ref = io.items = PTR
    return _set(io, kw)


def _llr_stats_io(**kw):
    io = _mcs(_grid(_lib.nrx_llr_stats_io(), num_heads=1, num_scales=1))
    io.scales[0] = 1.0
    io.llr = io.bits = io.mcs = io.active = io.loss = io.cnt = io.nonfinite = PTR
    return _set(io, kw)


def _chest3_io(**kw):
    io = _grid(_lib.nrx_chest3_io(), num_rx_ant=4, num_dmrs_symbols=2, no=0.1)
    io.dmrs_symbols[0], io.dmrs_symbols[1] = 2, 11
    io.cdm_group[0], io.cdm_group[1] = 0, 1
    for t in ("h_hat", "active", "h_out", "qh", "gf", "nu", "tcoef", "vconj", "lam", "vs", "mu"):
        setattr(io, t, PTR)
    return _set(io, kw)


def _gen_desc(**kw):
    d = _mcs(_grid(_lib.nrx_gen_desc(), num_rx_ant=4, num_dmrs_symbols=2))
    d.dmrs_symbols[0], d.dmrs_symbols[1] = 2, 11
    d.cdm_group[0], d.cdm_group[1] = 0, 1
    d.mcs_of_user[0], d.mcs_of_user[1] = 0, 2
    d.num_active, d.num_taps, d.num_sinusoids = 2, 4, 8
    d.max_delay_s, d.max_doppler_hz, d.subcarrier_spacing, d.no = 1e-7, 100.0, 30e3, 0.1
    d.seed, d.slot_offset = 1, 0
    return _set(d, kw)


def _size(fn, io):
    n = ctypes.c_size_t(0)
    rc = fn(ctypes.byref(io), ctypes.byref(n))
    return rc, n.value


# ---- nrx_count_errors -----------------------------------------------------------------------

COUNT_CASES = [
    (dict(llr=None), INVALID_ARG, b"null"), (dict(bits=None), INVALID_ARG, b"null"),
    (dict(active=None), INVALID_ARG, b"null"), (dict(counts=None), INVALID_ARG, b"null"),
    (dict(batch=0), SHAPE, b"shape"), (dict(num_tx=0), SHAPE, b"shape"), (dict(num_subcarriers=0), SHAPE, b"shape"),
    (dict(num_symbols=0), SHAPE, b"shape"), (dict(num_symbols=32), SHAPE, b"shape"),
    (dict(num_heads=0), SHAPE, b"shape"), (dict(num_heads=2), SHAPE, b"shape"),
    (dict(num_mcs=0), SHAPE, b"shape"), (dict(num_mcs=9), SHAPE, b"shape"),
    (dict(mcs_bits1=0), SHAPE, b"mcs_bits"), (dict(mcs_bits2=7), SHAPE, b"mcs_bits"),
    (dict(bits_stride=5), SHAPE, b"mcs_bits"),
]


@pytest.mark.parametrize("kw,code,word", COUNT_CASES)
def test_count_errors_argument_checks(lib, kw, code, word):
    io = _count_io(**kw)
    assert lib.nrx_count_errors(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()


def test_count_errors_null_io(lib):
    assert lib.nrx_count_errors(None, None) == INVALID_ARG
    assert b"null" in lib.nrx_last_error()


# ---- nrx_llr_demap --------------------------------------------------------------------------

def _demap(lib, **kw):
    a = dict(llr=PTR, batch=2, num_tx=2, num_subcarriers=12, num_symbols=14, bits_stride=6, bits=4, data_re=PTR,
             n_data=100, out=PTR)
    a.update(kw)
    return lib.nrx_llr_demap(a["llr"], a["batch"], a["num_tx"], a["num_subcarriers"], a["num_symbols"],
                             a["bits_stride"], a["bits"], a["data_re"], a["n_data"], a["out"], None)


DEMAP_CASES = [
    (dict(llr=None), INVALID_ARG, b"null"), (dict(data_re=None), INVALID_ARG, b"null"),
    (dict(out=None), INVALID_ARG, b"null"),
    (dict(batch=0), SHAPE, b"shape"), (dict(num_tx=0), SHAPE, b"shape"), (dict(num_subcarriers=0), SHAPE, b"shape"),
    (dict(num_symbols=0), SHAPE, b"shape"), (dict(bits=0), SHAPE, b"shape"), (dict(bits=7), SHAPE, b"shape"),
    (dict(n_data=0), SHAPE, b"shape"), (dict(n_data=12 * 14 + 1), SHAPE, b"shape"),
]


@pytest.mark.parametrize("kw,code,word", DEMAP_CASES)
def test_llr_demap_argument_checks(lib, kw, code, word):
    assert _demap(lib, **kw) == code
    assert word in lib.nrx_last_error()


# ---- nrx_compute_pe: the rejecting side (the values are checked in test_oracle / test_abi) ----

def _pe(lib, num_tx=2, F=12, T=14, dmrs=(2, 11), nsym=None, cdm=(0, 1), pe=True, null=()):
    sym = (ctypes.c_int32 * max(len(dmrs), 1))(*dmrs)
    grp = (ctypes.c_int32 * 16)(*cdm)
    out = (ctypes.c_float * (max(num_tx, 1) * max(F, 1) * max(T, 1) * 2))()
    return lib.nrx_compute_pe(num_tx, F, T, None if "dmrs" in null else sym, len(dmrs) if nsym is None else nsym,
                              None if "cdm" in null else grp, None if "pe" in null else out)


PE_CASES = [
    (dict(num_tx=0), b"argument"), (dict(F=0), b"argument"), (dict(T=0), b"argument"), (dict(nsym=0), b"argument"),
    (dict(null=("dmrs",)), b"argument"), (dict(null=("cdm",)), b"argument"), (dict(null=("pe",)), b"argument"),
    (dict(cdm=(0, 2)), b"cdm_group"), (dict(cdm=(-1, 0)), b"cdm_group"),
    (dict(F=1, cdm=(0, 1)), b"pilots"),          # group 1 owns the odd subcarriers: none of them at F = 1
]


@pytest.mark.parametrize("kw,word", PE_CASES)
def test_compute_pe_argument_checks(lib, kw, word):
    assert _pe(lib, **kw) == INVALID_ARG
    assert word in lib.nrx_last_error()
    assert _pe(lib) == OK


# ---- nrx_gen_workspace_size -----------------------------------------------------------------

GEN_CASES = [
    (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"),
    (dict(num_subcarriers=1), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_dmrs_symbols=0), SHAPE, b"num_dmrs_symbols"), (dict(num_dmrs_symbols=5), SHAPE, b"num_dmrs_symbols"),
    (dict(dmrs_symbols1=14), INVALID_ARG, b"dmrs_symbols"), (dict(dmrs_symbols0=-1), INVALID_ARG, b"dmrs_symbols"),
    (dict(dmrs_symbols1=2), INVALID_ARG, b"dmrs_symbols"),
    (dict(dmrs_symbol_mask=1 << 2), INVALID_ARG, b"dmrs_symbol_mask"),
    (dict(num_mcs=0), INVALID_ARG, b"num_mcs"), (dict(num_mcs=9), INVALID_ARG, b"num_mcs"),
    (dict(mcs_bits1=3), INVALID_ARG, b"mcs_bits"), (dict(mcs_bits0=8), INVALID_ARG, b"mcs_bits"),
    (dict(cdm_group0=2), INVALID_ARG, b"cdm_group"), (dict(cdm_group1=-1), INVALID_ARG, b"cdm_group"),
    (dict(mcs_of_user0=-2), INVALID_ARG, b"mcs_of_user"), (dict(mcs_of_user1=3), INVALID_ARG, b"mcs_of_user"),
    (dict(num_active=0), INVALID_ARG, b"num_active"), (dict(num_active=3), INVALID_ARG, b"num_active"),
    (dict(num_taps=0), INVALID_ARG, b"num_taps"), (dict(num_taps=9), INVALID_ARG, b"num_taps"),
    (dict(num_sinusoids=0), INVALID_ARG, b"num_sinusoids"), (dict(num_sinusoids=17), INVALID_ARG, b"num_sinusoids"),
    (dict(max_delay_s=-1e-9), INVALID_ARG, b"finite"), (dict(max_delay_s=float("nan")), INVALID_ARG, b"finite"),
    (dict(max_doppler_hz=-1.0), INVALID_ARG, b"finite"), (dict(subcarrier_spacing=0.0), INVALID_ARG, b"finite"),
    (dict(no=-0.1), INVALID_ARG, b"finite"), (dict(no=float("nan")), INVALID_ARG, b"finite"),
    (dict(slot_offset=-1), INVALID_ARG, b"slot_offset"),
]


@pytest.mark.parametrize("kw,code,word", GEN_CASES)
def test_gen_argument_checks(lib, kw, code, word):
    d = _gen_desc(**kw)
    assert _size(lib.nrx_gen_workspace_size, d)[0] == code
    assert word in lib.nrx_last_error()
    o = _lib.nrx_gen_out()
    o.y = PTR
    assert lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), PTR, BIG, None) == code


def test_gen_null_arguments_and_workspace(lib):
    d = _gen_desc()
    rc, need = _size(lib.nrx_gen_workspace_size, d)
    assert rc == OK and need > 0
    assert _size(lib.nrx_gen_workspace_size, _gen_desc(mcs_of_user1=-1, no=0.0, max_delay_s=0.0))[0] == OK
    n = ctypes.c_size_t(0)
    assert lib.nrx_gen_workspace_size(None, ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_gen_workspace_size(ctypes.byref(d), None) == INVALID_ARG
    o = _lib.nrx_gen_out()
    o.y = PTR
    assert lib.nrx_generate_slots(ctypes.byref(d), None, PTR, BIG, None) == INVALID_ARG
    assert lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), None, BIG, None) == INVALID_ARG
    assert b"null" in lib.nrx_last_error()
    assert lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), PTR, need - 1, None) == WORKSPACE
    assert b"workspace too small" in lib.nrx_last_error() and str(need).encode() in lib.nrx_last_error()
    o.bits, o.bits_stride = PTR, 5
    assert lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), PTR, BIG, None) == SHAPE
    assert b"bits_stride" in lib.nrx_last_error()
    o.bits_stride, o.y_real = 6, PTR
    assert lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), PTR, BIG, None) == INVALID_ARG
    assert b"pairs" in lib.nrx_last_error()
    o.y_real = None
    o.h_ls_real = o.h_ls_imag = PTR
    d18 = _gen_desc(num_subcarriers=18)
    assert lib.nrx_generate_slots(ctypes.byref(d18), ctypes.byref(o), PTR, BIG, None) == SHAPE
    assert b"num_subcarriers" in lib.nrx_last_error()


# ---- what test_lmmse_ref.py and test_chest_ref.py leave out ------------------------------------

LMMSE_CASES = [
    (dict(batch=65536), SHAPE, b"batch"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(no=float("inf")), INVALID_ARG, b"no must"), (dict(err_var=float("nan")), INVALID_ARG, b"err_var"),
    (dict(err_var=float("inf")), INVALID_ARG, b"err_var"), (dict(mcs_bits1=1), INVALID_ARG, b"mcs_bits"),
]


@pytest.mark.parametrize("kw,code,word", LMMSE_CASES)
def test_lmmse_argument_checks(lib, kw, code, word):
    io = _lmmse_io(**kw)
    assert lib.nrx_lmmse_detect(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()


COV_CASES = [
    (dict(h=None), INVALID_ARG, b"null"), (dict(acc=None), INVALID_ARG, b"null"),
    (dict(num_symbols=15), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
]


@pytest.mark.parametrize("kw,code,word", COV_CASES)
def test_cov_argument_checks(lib, kw, code, word):
    """the frequency / time and the spatial accumulators take the same fields and the same rules, in the
    sizing call as in the launch"""
    for cls, size, run in ((_lib.nrx_cov_io, lib.nrx_cov_workspace_size, lib.nrx_cov_accumulate),
                           (_lib.nrx_cov_space_io, lib.nrx_cov_space_workspace_size, lib.nrx_cov_space_accumulate)):
        io = _cov_io(cls, **kw)
        assert _size(size, io)[0] == code
        assert word in lib.nrx_last_error()
        assert run(ctypes.byref(io), PTR, BIG, None) == code
        assert word in lib.nrx_last_error()


def test_cov_null_io_bytes_and_workspace(lib):
    n = ctypes.c_size_t(0)
    for cls, size, run in ((_lib.nrx_cov_io, lib.nrx_cov_workspace_size, lib.nrx_cov_accumulate),
                           (_lib.nrx_cov_space_io, lib.nrx_cov_space_workspace_size, lib.nrx_cov_space_accumulate)):
        io = _cov_io(cls)
        assert size(None, ctypes.byref(n)) == INVALID_ARG
        assert size(ctypes.byref(io), None) == INVALID_ARG
        assert run(None, PTR, BIG, None) == INVALID_ARG
        rc, need = _size(size, io)
        assert rc == OK and need > 0
        assert run(ctypes.byref(io), None, BIG, None) == INVALID_ARG
        assert b"null" in lib.nrx_last_error() and b"workspace" in lib.nrx_last_error()
        assert run(ctypes.byref(io), PTR, need - 1, None) == WORKSPACE
        assert b"workspace too small" in lib.nrx_last_error() and str(need).encode() in lib.nrx_last_error()


# ---- rules that differ between entry points on purpose ---------------------------------------

def test_num_tx_above_8_is_unsupported_by_the_detectors_only(lib):
    io = _lmmse_io(num_tx=9)
    assert lib.nrx_lmmse_detect(ctypes.byref(io), None) == UNSUPPORTED and b"num_tx" in lib.nrx_last_error()
    kio = _kbest_io(num_tx=9)
    assert lib.nrx_kbest_detect(ctypes.byref(kio), PTR, BIG, None) == UNSUPPORTED and b"num_tx" in lib.nrx_last_error()
    assert _size(lib.nrx_kbest_workspace_size, kio)[0] == UNSUPPORTED
    assert _size(lib.nrx_cov_workspace_size, _cov_io(num_tx=9))[0] == OK
    assert _size(lib.nrx_nmse_workspace_size, _nmse_io(num_tx=9))[0] == OK
    assert _size(lib.nrx_cov_workspace_size, _cov_io(num_tx=16))[0] == OK
    assert _size(lib.nrx_kbest_workspace_size, _kbest_io(num_tx=8))[0] == OK


def test_num_mcs_out_of_range_is_invalid_arg_for_the_generator_and_shape_elsewhere(lib):
    for bad in (0, 9):
        assert _size(lib.nrx_gen_workspace_size, _gen_desc(num_mcs=bad))[0] == INVALID_ARG
        assert b"num_mcs" in lib.nrx_last_error()
        io = _lmmse_io(num_mcs=bad)
        assert lib.nrx_lmmse_detect(ctypes.byref(io), None) == SHAPE and b"num_mcs" in lib.nrx_last_error()
        assert _size(lib.nrx_llr_stats_workspace_size, _llr_stats_io(num_mcs=bad))[0] == SHAPE
        assert b"num_mcs" in lib.nrx_last_error()


def test_one_subcarrier_is_rejected_by_the_generator_only(lib):
    assert _size(lib.nrx_gen_workspace_size, _gen_desc(num_subcarriers=1))[0] == SHAPE
    assert b"num_subcarriers" in lib.nrx_last_error()
    assert _size(lib.nrx_gen_workspace_size, _gen_desc(num_subcarriers=2))[0] == OK
    assert _size(lib.nrx_cov_workspace_size, _cov_io(num_subcarriers=1))[0] == OK
    assert _size(lib.nrx_nmse_workspace_size, _nmse_io(num_subcarriers=1))[0] == OK


def test_three_bits_per_symbol_are_legal_for_the_soft_metrics_only(lib):
    io = _lmmse_io(mcs_bits1=3)
    assert lib.nrx_lmmse_detect(ctypes.byref(io), None) == INVALID_ARG and b"mcs_bits" in lib.nrx_last_error()
    assert _size(lib.nrx_kbest_workspace_size, _kbest_io(mcs_bits1=3))[0] == INVALID_ARG
    assert b"mcs_bits" in lib.nrx_last_error()
    assert _size(lib.nrx_gen_workspace_size, _gen_desc(mcs_bits1=3))[0] == INVALID_ARG
    assert b"mcs_bits" in lib.nrx_last_error()
    assert _size(lib.nrx_llr_stats_workspace_size, _llr_stats_io(mcs_bits1=3))[0] == OK
    assert _size(lib.nrx_llr_stats_workspace_size, _llr_stats_io(mcs_bits1=1, mcs_bits2=8, bits_stride=8))[0] == OK


def _ldpc_handle(lib):
    import numpy as np
    shifts = np.full((4, 8), -1, np.int16)
    for i in range(4):
        shifts[i, i] = 1
        shifts[i, i + 1] = 0
    shifts[0, 5:] = 0
    code = _lib.nrx_ldpc_code()
    code.mb, code.nb, code.z, code.kb = 4, 8, 8, 4
    code.shifts = shifts.ctypes.data
    h = ctypes.c_void_p()
    assert lib.nrx_ldpc_create(ctypes.byref(code), -1, ctypes.byref(h)) == OK
    return h


def test_workspace_alignment_per_entry_point(lib):
    """each launch asks for the alignment its kernels' widest workspace access needs: none for the
    covariance accumulators, 4 bytes for the 3-D estimator, 8 for the soft metrics, 16 for K-best and
    LDPC.  A pointer that passes is taken as far as the size check."""
    def outcome(run, io, ptr, need):
        rc = run(ctypes.byref(io), ptr, need - 1, None)
        assert rc in (INVALID_ARG, WORKSPACE)
        assert (b"aligned" if rc == INVALID_ARG else b"workspace too small") in lib.nrx_last_error()
        return rc

    def aligned_to(run, io, need):
        """the smallest power of two whose multiples the entry point takes"""
        assert outcome(run, io, PTR, need) == WORKSPACE
        for a in (1, 2, 4, 8, 16, 32):
            if outcome(run, io, PTR + a, need) == WORKSPACE:
                assert all(outcome(run, io, PTR + k * a, need) == WORKSPACE for k in (3, 5))
                return a
        raise AssertionError("no alignment up to 32 bytes is accepted")

    for io, size, run, align in (
            (_cov_io(), lib.nrx_cov_workspace_size, lib.nrx_cov_accumulate, 1),
            (_cov_io(_lib.nrx_cov_space_io), lib.nrx_cov_space_workspace_size, lib.nrx_cov_space_accumulate, 1),
            (_chest3_io(), lib.nrx_chest3_workspace_size, lib.nrx_chest_lmmse3, 4),
            (_llr_stats_io(), lib.nrx_llr_stats_workspace_size, lib.nrx_llr_stats, 8),
            (_nmse_io(), lib.nrx_nmse_workspace_size, lib.nrx_chest_nmse, 8),
            (_kbest_io(), lib.nrx_kbest_workspace_size, lib.nrx_kbest_detect, 16)):
        rc, need = _size(size, io)
        assert rc == OK and need > 1
        assert aligned_to(run, io, need) == align, run.__name__
    h = _ldpc_handle(lib)
    io = _lib.nrx_ldpc_io()
    io.num_cw, io.num_iter, io.cn_type, io.early_stop, io.ms_scale, io.llr_clip = 3, 20, 0, 1, 0.75, 20.0
    io.llr_in = io.skip = io.hard = io.app = io.iters = io.parity_ok = PTR
    n = ctypes.c_size_t(0)
    assert lib.nrx_ldpc_workspace_size(h, ctypes.byref(io), ctypes.byref(n)) == OK
    assert aligned_to(lambda *a: lib.nrx_ldpc_decode(h, *a), io, n.value) == 16
    lib.nrx_ldpc_destroy(h)
