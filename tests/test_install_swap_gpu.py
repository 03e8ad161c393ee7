"""The INTEGRATION.md §2 import swap itself: after friture_amd.backend_swap.install() the reference's own import lines
resolve to the HIP-backed classes, and the logic of the reference's unit test of the octave banks
(friture/test/test_octave_filters.py:37-100) passes against them.

The suite stands alone: the swap hangs on empty `friture` / `friture.signal` packages, and the upstream test's three methods are
replayed through the same `from friture... import` lines.  Every call lands in libfriture_hip.so."""
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def swapped(hip):
    from friture_amd import backend_swap
    created = []
    for name in ("friture", "friture.signal"):                  # an empty package to hang the swap on
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
            created.append(name)
    backend_swap.install()
    yield
    backend_swap.uninstall()
    for name in created:
        sys.modules.pop(name, None)


def test_reference_import_lines_resolve_to_the_hip_backend(swapped):
    import friture_amd.audioproc
    import friture_amd.filter
    import friture_amd.octavefilters
    from friture.audioproc import audioproc
    from friture.filter import octave_filter_bank_decimation, octave_filter_bank_decimation_filtic
    from friture.octavefilters import NOCTAVE, Octave_Filters
    from friture.signal.correlation import generalized_cross_correlation
    from friture.signal.decimate import decimate_multiple
    assert audioproc is friture_amd.audioproc.audioproc and Octave_Filters is friture_amd.octavefilters.Octave_Filters
    assert octave_filter_bank_decimation is friture_amd.filter.octave_filter_bank_decimation and NOCTAVE == 9
    assert octave_filter_bank_decimation_filtic.__module__ == "friture_amd.filter"
    assert generalized_cross_correlation.__module__ == "friture_amd.signal.correlation"
    assert decimate_multiple.__module__ == "friture_amd.signal.decimate"
    # and a call through the swapped name reaches the device
    p = audioproc()
    p.set_fftsize(1024)
    x = np.random.default_rng(3).standard_normal(1024)
    from oracle import dsp
    ref = dsp.psd_frame(x, dsp.hann_symmetric(1024))
    assert np.max(np.abs(p.analyzelive(x) - ref)) <= 1e-12 * np.max(ref)


def test_upstream_octave_filter_logic_through_the_swap(swapped):
    """friture/test/test_octave_filters.py:37-100 replayed through the swapped import lines: accumulated band energies of
    the FFT bank within 5 % of the exact IIR bank's over 8 blocks of default_rng(42) noise for bpo 1, 6, 12, 24; the
    decimation factors' ordering; one default_rng(123) block of the undecimated octave within 10 % max-abs / 5 % energy."""
    from friture.filter import octave_filter_bank_decimation, octave_filter_bank_decimation_filtic
    from friture.octavefilters import NOCTAVE, Octave_Filters
    for bpo in (1, 6, 12, 24):
        ofs = Octave_Filters(bpo)
        x = np.random.default_rng(42).standard_normal(8 * 1024)
        zis = octave_filter_bank_decimation_filtic(ofs.bdec, ofs.adec, ofs.boct, ofs.aoct)
        e_iir, e_fft = np.zeros(NOCTAVE * bpo), np.zeros(NOCTAVE * bpo)
        for b in range(8):
            xb = x[b * 1024:(b + 1) * 1024]
            y_i, dec_i, zis = octave_filter_bank_decimation(ofs.bdec, ofs.adec, ofs.boct, ofs.aoct, xb, zis)
            y_f, dec_f = ofs.filter(xb)
            assert list(dec_f) == list(dec_i) == list(ofs.get_decs())
            if b >= 2:
                e_iir += [np.sum(np.asarray(v) ** 2) for v in y_i]
                e_fft += [np.sum(np.asarray(v) ** 2) for v in y_f]
        assert np.all(np.abs(e_fft / e_iir - 1.0) < 0.05), (bpo, e_fft / e_iir)
        dec = list(ofs.get_decs())
        assert dec[0] == 256 and dec[-1] == 1 and all(dec[i] >= dec[i + 1] for i in range(len(dec) - 1))
    ofs = Octave_Filters(3)
    x = np.random.default_rng(123).standard_normal(1024)
    zis = octave_filter_bank_decimation_filtic(ofs.bdec, ofs.adec, ofs.boct, ofs.aoct)
    y_i, _, _ = octave_filter_bank_decimation(ofs.bdec, ofs.adec, ofs.boct, ofs.aoct, x, zis)
    y_f, _ = ofs.filter(x)
    for a, b in zip(y_f[-3:], y_i[-3:]):
        a, b = np.asarray(a), np.asarray(b)
        assert np.max(np.abs(a - b)) < 0.10 * np.max(np.abs(b)) and abs(np.sum(a ** 2) / np.sum(b ** 2) - 1) < 0.05
