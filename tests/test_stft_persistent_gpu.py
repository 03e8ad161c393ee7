"""The walk of the float32 N = 1024 STFT instances (stft_wave.h, PERSIST; frt_stft_set_persistent): a grid of resident workgroups
whose wavefronts load their constants once and stride over runs of frames.  It must give, bit for bit, what the launch of
one run of 16 frames per lane group gives: rows and Nyquist plane, colour and PSD kinds, split and packed rows.  One case is also
held against oracle/dsp.py at the bars of tests/test_eight_bin_epilogue_gpu.py, whose input this module uses: bins 512 and 256
walk along colour-index edges frame by frame and the first half-frames are silent, so a frame that took its samples, its row or
its Nyquist lane from the wrong side of a run boundary shows as colour.

Every shape comes twice: with runs of 4 frames (set_run_length(4) is the walk's run length under set_persistent(1, ...)), the
smallest shapes that can go wrong, and with the run length the library ships (WALK_RUN = kWalkRun of stft_launch, no run length set)."""
import functools

import numpy as np
import pytest

import test_eight_bin_epilogue_gpu as eight

N, HOP, M = eight.N, eight.HOP, eight.M
WALK_RUN = 16
RUNS = [4, WALK_RUN]
SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def case():
    return eight.build_case()


def long_signal(channel, frames, hop=HOP):
    """the module's signal repeated until it holds `frames` frames (the seams are ordinary data: the comparison is bitwise)"""
    period = case()["x"][channel, :eight.F_ALL * HOP]
    need = N + hop * (frames - 1)
    return np.tile(period, need // period.size + 1)[:need]


class Engine:
    """one configured engine: classic (one run of 16 frames per lane group) or the walk"""

    def __init__(self, hop, channels, mode, blocks=0, run=None):
        from friture_amd.stft import StftEngine
        self.eng = StftEngine(N, hop, channels, 32)
        self.eng.set_epilogue(case()["weight"], eight.SPEC_MIN, eight.SPEC_MAX, case()["lut"])
        if mode == "classic":
            self.eng.set_persistent(0, 0)
            self.eng.set_run_length(16)
        else:
            self.eng.set_run_length(0 if run is None else run)
            self.eng.set_persistent(mode, blocks)

    def outputs(self, xd, kinds, layouts=("split", "packed"), tail=0):
        """-> {(kind, layout): uint32 array [C, F (+ tail), M + 1]}; the buffers are pre-filled with SENTINEL, `tail` rows longer than
        the frames (one channel only: the tail lies behind the last row)"""
        import torch
        C, F = xd.shape[0], self.eng.frames_for(xd.shape[1])
        assert tail == 0 or C == 1
        out = {}
        for kind in kinds:
            dt = torch.int32 if kind == 3 else torch.float32
            for layout in layouts:
                if layout == "split":
                    rows = torch.full((C, F + tail, M), SENTINEL, dtype=torch.int32, device=xd.device).view(dt)
                    nyq = torch.full((C, F + tail), SENTINEL, dtype=torch.int32, device=xd.device).view(dt)
                    self.eng.run_split(kind, xd, rows, nyq)
                    got = torch.cat([rows, nyq[..., None]], dim=-1)
                else:
                    got = torch.full((C, F + tail, M + 1), SENTINEL, dtype=torch.int32, device=xd.device).view(dt)
                    self.eng.run(kind, xd, got)
                torch.cuda.synchronize()
                out[(kind, layout)] = got.view(torch.int32).cpu().numpy().view(np.uint32)
        return out

    def close(self):
        self.eng.close()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def compare(x, hop, blocks, mode=1, tail=0, run=WALK_RUN):
    """walk against classic, every kind and layout; -> the walk's outputs"""
    import torch

    from friture_amd import _lib
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    kinds = (_lib.FRT_STFT_IMAGE, _lib.FRT_STFT_PSD)
    classic, walk = Engine(hop, x.shape[0], "classic"), Engine(hop, x.shape[0], mode, blocks, None if run == WALK_RUN else run)
    want, got = classic.outputs(xd, kinds, tail=tail), walk.outputs(xd, kinds, tail=tail)
    classic.close()
    walk.close()
    for key in want:
        assert same_bits(got[key], want[key]), f"kind {key[0]}, {key[1]} rows: the walk differs from the classic launch"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("hop", [512, 256])
def test_uneven_trips_and_a_short_last_run(hip, hop, run):
    """9 runs and one frame on two workgroups (37 frames in runs of 4): ten runs for eight waves — two waves walk twice — and the
    last run holds one frame.  hop 512 is the instance that fetches the next run's first frame in its last frame, hop 256 the one
    that drains between runs.  The hop 512 result in runs of 4 is also the oracle's, at the bars of the eight-value epilogue's tests."""
    from friture_amd import _lib
    first, count = 14, 9 * run + 1
    x = eight.frames_of(case()["x"][:1], first, count, N, hop) if run == 4 else long_signal(0, count, hop)[None, :]
    got = compare(x, hop, 2, run=run)
    assert got[(_lib.FRT_STFT_IMAGE, "split")].shape == (1, count, M + 1)
    if hop == HOP and run == 4:
        ref = case()["ref"][:1, first:first + count]
        psd = got[(_lib.FRT_STFT_PSD, "split")].view(np.float32)
        eight.assert_parity(got[(_lib.FRT_STFT_IMAGE, "split")], psd, ref, case()["weight"], case()["lut"])
        eight.assert_psd(psd, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
def test_runs_cross_channels_inside_one_walk(hip, run):
    """three channels of two runs and a frame (nine frames in runs of 4, 4 and 1) on ONE workgroup: every wave's walk crosses channel
    boundaries, the channel stride of the samples (N + 8 hop) is not the frames' (9 hop), and the Nyquist plane is written channel by channel"""
    f = 2 * run + 1
    x = np.concatenate([eight.frames_of(case()["x"][:1], 20, f), eight.frames_of(case()["x"][1:], 20, f), eight.frames_of(case()["x"][:1], 31, f)])
    assert x.shape == (3, N + (f - 1) * HOP)
    compare(x, HOP, 1, run=run)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
def test_idle_waves_write_nothing(hip, run):
    """a run and a frame (five frames in runs of 4) are two runs; four workgroups are sixteen waves: fourteen idle.  Nothing behind
    the last row changes."""
    f = run + 1
    got = compare(eight.frames_of(case()["x"][:1], 30, f), HOP, 4, tail=8, run=run)
    for key, arr in got.items():
        assert arr.shape[1] == f + 8 and np.all(arr[:, f:] == SENTINEL), f"{key}: written behind the last row"
        assert not np.all(arr[:, :f] == SENTINEL)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
def test_three_trips_each_and_one_wave_a_fourth(hip, run):
    blocks = 3
    frames = 3 * run * (4 * blocks) + 1
    compare(long_signal(0, frames)[None, :], HOP, blocks, run=run)


@pytest.mark.gpu
def test_automatic_choice_keeps_small_batches_classic(hip):
    """1000 frames give the resident waves far fewer than four runs each: set_persistent(-1, 0) launches one run per lane group"""
    compare(long_signal(1, 1000)[None, :], HOP, 0, mode=-1)


@pytest.mark.gpu
def test_automatic_choice_takes_the_walk_on_a_large_batch(hip):
    """sixteen frames for every resident wave (three workgroups of four waves per CU at most: three waves per SIMD) and three frames
    more — four runs of four, or the one run of WALK_RUN that the automatic choice asks for: it walks.  Compared on the device; the
    first, the last and 64 seeded runs are compared once more on the host, bit for bit."""
    import torch

    from friture_amd import _lib
    resident = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    frames = 4 * 4 * 4 * resident + 3
    period = torch.from_numpy(case()["x"][0, :eight.F_ALL * HOP].copy()).cuda()
    need = N + HOP * (frames - 1)
    xd = period.repeat(need // period.numel() + 1)[:need][None, :].contiguous()
    classic, walk = Engine(HOP, 1, "classic"), Engine(HOP, 1, -1)
    runs = (frames + WALK_RUN - 1) // WALK_RUN
    picks = np.unique(np.concatenate([[0, runs - 1], np.random.default_rng(11).integers(0, runs, 64)]))
    for kind in (_lib.FRT_STFT_IMAGE, _lib.FRT_STFT_PSD):
        dt = torch.int32 if kind == _lib.FRT_STFT_IMAGE else torch.float32
        res = []
        for e in (classic, walk):
            rows = torch.full((1, frames, M), SENTINEL, dtype=torch.int32, device="cuda").view(dt)
            nyq = torch.full((1, frames), SENTINEL, dtype=torch.int32, device="cuda").view(dt)
            e.eng.run_split(kind, xd, rows, nyq)
            res.append((rows.view(torch.int32), nyq.view(torch.int32)))
        torch.cuda.synchronize()
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), f"kind {kind}"
        for r in picks:
            lo, hi = r * WALK_RUN, min((r + 1) * WALK_RUN, frames)
            for want, got in zip(res[0], res[1]):
                assert same_bits(got[:, lo:hi].cpu().numpy(), want[:, lo:hi].cpu().numpy()), f"kind {kind}, run {r}"
    classic.close()
    walk.close()


@pytest.mark.gpu
def test_prepared_launch_walks_like_run_split(hip):
    import torch

    from friture_amd import _lib
    xd = torch.from_numpy(eight.frames_of(case()["x"][:1], 14, 37)).cuda()
    walk = Engine(HOP, 1, 1, 2)
    for kind in (_lib.FRT_STFT_IMAGE, _lib.FRT_STFT_PSD):
        dt = torch.int32 if kind == _lib.FRT_STFT_IMAGE else torch.float32
        rows, nyq = walk.eng.run_split(kind, xd)
        prows = torch.full((1, 37, M), SENTINEL, dtype=torch.int32, device="cuda").view(dt)
        pnyq = torch.full((1, 37), SENTINEL, dtype=torch.int32, device="cuda").view(dt)
        launch = walk.eng.prepare(kind, xd, prows, pnyq)
        launch()
        torch.cuda.synchronize()
        assert torch.equal(rows.view(torch.int32), prows.view(torch.int32)) and torch.equal(nyq.view(torch.int32), pnyq.view(torch.int32))
    walk.close()
