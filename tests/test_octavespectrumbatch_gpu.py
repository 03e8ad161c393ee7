"""OctaveSpectrumBatch on the GPU (octspecbatch.hip over the FFT overlap-add bank) against the numpy replay of the widget's chain
(oracle/octavespectrumbatch.py, pinned to the reference by tests/golden/octavespectrumbatch.npz) and against itself.

Bars, the project's own for this bank (tests/test_ola_gpu.py): energies |got - want| <= 1e-10 want + 1e-20 max(want); dB against
10 log10(energy_got + 1e-30) + w formed in numpy from the returned energies: 1e-12 absolute (a few ulp at magnitudes up to 300)."""
import numpy as np
import pytest

from oracle import octavespectrumbatch as H

pytestmark = pytest.mark.gpu
T0 = 8192 + 768         # crosses the bank's 3072-output set at stages 0 and 1 and leaves a pending remainder


def batch_for(bpo=3, weighting=1):
    from friture_amd.octavespectrum import OctaveSpectrumBatch
    return OctaveSpectrumBatch(bpo, weighting)


def to_np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def check(res, want_energy, w, what=""):
    """energy against the replay's rows, db against numpy's read-out of the returned energy; prints both figures first."""
    energy, db = to_np(res.energy), to_np(res.db)
    worst = H.energy_close(energy, want_energy)
    worst_db = float(np.max(np.abs(db - H.db_of(energy, w)))) if db.size else 0.0
    print(f"{what}: energy {worst:.3e} of the bar, dB {worst_db:.3e} absolute")
    assert worst <= 1.0 and worst_db <= 1e-12, (what, worst, worst_db)


@pytest.mark.parametrize("bpo,weighting,dtype,device", [(1, 0, "float32", "numpy"), (3, 2, "float64", "cuda"), (3, 0, "float32", "cuda"),
                                                       (6, 2, "float64", "numpy"), (6, 0, "float32", "cuda")])
def test_parity_with_the_replay_mixed_chunk_lengths(hip, bpo, weighting, dtype, device):
    """S = 2, chunk lengths drawn from {256, 512, 768, 1024}; bpo 6 goes through the bank's deferred band-filter launch."""
    import torch
    x, ends, ref = H.case(2, T0, bpo, weighting, 11)
    assert T0 - ends[-1] > 0 and len(set(np.diff(ends).tolist())) == 4
    xin = x.astype(dtype)                                            # float64 of float32 values: the replay's own samples
    if device == "cuda":
        xin = torch.from_numpy(xin).cuda()
    res = batch_for(bpo, weighting).run(xin, ends=ends, with_energy=True)
    assert (device == "cuda") == hasattr(res.db, "is_cuda") and res.db.shape == (2, len(ends), 9 * bpo)
    assert str(res.db.dtype).endswith("float64") and str(res.state.samples.dtype).endswith("float64")
    check(res, ref["energy"], H.band_weight(bpo, weighting), f"bpo {bpo} {dtype} {device}")
    assert res.state.pending == T0 - ends[-1] and np.array_equal(to_np(res.state.samples), x[:, ends[-1]:].astype(np.float64))
    assert np.array_equal(res.ends, ends) and len(res.f_nominal) == 9 * bpo
    assert H.energy_close(to_np(res.state.energies), ref["energy"][:, -1]) <= 1.0


def test_two_level_walk(hip):
    """T = 4 * 64 * 256 + 1024 with mixed chunk lengths: at least 4 * 64 sub-blocks are consumed, the count from which the walk
    is split into runs of 64 (a local launch, then the chained one), and fewer than 5 * 64, so the last run is ragged."""
    from friture_amd.octavespectrum import OctaveSpectrumBatch
    T = 4 * 64 * 256 + 1024
    x, ends, ref = H.case(1, T, 3, 1, 21)
    assert ends[-1] // 256 >= 4 * 64
    res = OctaveSpectrumBatch(3).run(x, ends=ends, with_energy=True)
    check(res, ref["energy"], H.band_weight(3, 1), "two-level")


def test_lowest_stage_crosses_a_set_boundary(hip):
    x, ends, ref = H.case(1, 3072 * 256 + 2048, 1, 1, 31, chunk=1024)
    res = batch_for(1).run(x[0], chunk=1024, with_energy=True)        # the stream axis left out
    assert res.db.shape == (len(ends), 9) and np.array_equal(res.ends, ends)
    check(res._replace(energy=res.energy[None], db=res.db[None]), ref["energy"], H.band_weight(1, 1), "long")


@pytest.mark.parametrize("cuts", [(5,), (5.5,), (3.5, 9)])
def test_pieces_equal_the_whole_to_rounding(hip, cuts):
    """Split at a chunk end, in the middle of a chunk (pending samples carried), and in three pieces: each piece against the
    replay of the whole at the same bars.  Not bit for bit: the bank's overlap-add sets of 3072 outputs start with each call, so
    the same products are summed in another order."""
    x, ends, ref = H.case(2, T0, 3, 1, 11)
    batch, state, start, row = batch_for(3), None, 0, 0
    marks = [int(ends[int(c)]) + (130 if c != int(c) else 0) for c in cuts] + [T0]
    for mark in marks:
        piece_ends = ends[row:np.searchsorted(ends, mark, "right")]
        res = batch.run(x[:, start:mark], ends=piece_ends - start, state=state, with_energy=True)
        n = len(piece_ends)
        check(res, ref["energy"][:, row:row + n], H.band_weight(3, 1), f"piece to {mark}")
        state, start, row = res.state, mark, row + n
        assert state.pending == mark - (int(piece_ends[-1]) if n else 0)
    assert row == len(ends)


def test_slabs(hip):
    x, ends, ref = H.case(2, T0, 3, 1, 11)
    batch = batch_for(3)
    res = batch.run(x[:, :8192], ends=ends[ends <= 8192], with_energy=True, scratch_bytes=100_000)
    assert batch.last_slabs >= 3
    check(res, ref["energy"][:, :len(res.ends)], H.band_weight(3, 1), f"{batch.last_slabs} slabs")


def test_keep_last_state_and_the_handle_as_a_cache(hip):
    import torch
    x, ends, ref = H.case(2, T0, 3, 1, 11)
    xd = torch.from_numpy(x).cuda()
    batch = batch_for(3)
    full = batch.run(xd, ends=ends, with_energy=True)
    last = batch.run(xd, ends=ends, keep="last", with_energy=True)
    assert last.db.shape == (2, 1, 27)
    assert torch.equal(last.db, full.db[:, -1:]) and torch.equal(last.energy, full.energy[:, -1:])
    for a, b in zip(last.state[:3], full.state[:3]):
        assert torch.equal(a, b)
    # a fresh run after other runs on the same object = a run on a new object: the handle is only a cache
    other = batch_for(3).run(xd, ends=ends, with_energy=True)
    assert torch.equal(other.db, full.db) and torch.equal(other.energy, full.energy) and torch.equal(other.state.tails, full.state.tails)
    # the caller's state is not modified
    first = batch.run(x[:, :4096 + 100], chunk=512)
    kept = [np.array(a, copy=True) for a in first.state[:3]]
    batch.run(x[:, 4096 + 100:], chunk=512, state=first.state)
    assert all(np.array_equal(a, b) for a, b in zip(kept, first.state[:3])) and first.state.pending == 100


def test_db_rows_are_what_curvebatch_reads(hip):
    """CurveBatch over result.db against HistPlot.setdata fed the per-refresh rows, bit for bit: the layouts meet."""
    import torch
    from friture_amd.plotcurves import CurveBatch, HistPlot
    x, ends, _ = H.case(2, T0, 3, 1, 11)
    res = batch_for(3).run(torch.from_numpy(x).cuda(), ends=ends)
    assert res.db.is_contiguous()
    curves = CurveBatch(-100., -20.).run(res.db)
    db = res.db.cpu().numpy()
    for s in range(2):
        plot = HistPlot()
        plot.setspecrange(-100., -20.)
        for r in range(len(ends)):
            plot.setdata(res.flow, res.fhigh, res.f_nominal, db[s, r])
            got = [to_np(curves[i][s, r]) for i in range(4)]
            assert all(np.array_equal(g, w) for g, w in zip(got, (plot.signal[2], plot.signal[3], plot.peak[2], plot.peak[3]))), (s, r)


def test_edge_cases(hip):
    batch = batch_for(3, 1)
    x, _, _ = H.case(2, T0, 3, 1, 11)
    # shorter than a chunk: no refresh, everything pending, the state carried
    res = batch.run(x[:, :300], chunk=512)
    assert res.db.shape == (2, 0, 27) and res.state.pending == 300 and np.array_equal(res.state.samples, x[:, :300].astype(np.float64))
    assert not res.state.energies.any() and not res.state.tails.any()
    nxt = batch.run(x[:, 300:1024], chunk=512, state=res.state, with_energy=True)
    assert nxt.db.shape == (2, 2, 27) and nxt.state.pending == 0
    whole = batch.run(x[:, :1024], chunk=512, with_energy=True)
    assert H.energy_close(nxt.energy, whole.energy) <= 1.0
    # a call of one 256-sample chunk: the bank is asked for one sub-block only
    tiny = batch.run(x[:, :256], chunk=256, with_energy=True)
    check(tiny, H.replay(x[:, :256].astype(np.float64), [256], 3, 1)["energy"], H.band_weight(3, 1), "one sub-block")
    # silence: sp = 0 exactly, dB = 10 log10(1e-30) + w
    zero = batch.run(np.zeros((1, 2048), np.float32), chunk=512, with_energy=True)
    assert not zero.energy.any()
    print("silence: largest |dB - (-300 + w)|", float(np.max(np.abs(zero.db - (-300.0 + H.band_weight(3, 1))))))
    assert np.array_equal(zero.db, np.broadcast_to(-300.0 + H.band_weight(3, 1), (1, 4, 27)))
    # one stream without its axis
    one = batch.run(x[0, :2048], chunk=1024, with_energy=True)
    assert one.db.shape == (2, 27) and one.state.energies.shape == (1, 27)
    assert H.energy_close(one.energy[None], batch.run(x[:1, :2048], chunk=1024, with_energy=True).energy) <= 1.0
    with pytest.raises(ValueError, match="chunk 0 has 100 samples"):
        batch.run(x, ends=[100])
