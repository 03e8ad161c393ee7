"""The LDS image of pcm_encode_kernel (csrc/pcmenc.hip) against the bank rules of gfx950, on the CPU: the sibling of
test_pcm_lds_layout.py.  tools/exp/lds_layout_model.py pcm_encode restates the layout the kernel writes and reads through —
pcm.hip's pads, pcmenc_phys(D) = D + (D >> 5) + (D >> 10) on logical dwords — and counts the distinct addresses that meet on one
bank per lane group: for the sample writes of phase 1 (lane stride channels * width bytes; sub-dword stores counted with the
lanes of one dword as one address, and with every byte apart) and for the four dword reads per thread of phase 2.  What
DESIGN.md R3 quotes is asserted here for every format x channels in (1, 2, 3, 6, 8, 32, 64) x destination address mod 16 in (0, 1,
3, 8): no write is worse than 3-way where the flat image would serialise up to a whole lane group, and the drain reads are
conflict free for an aligned destination and 2-way otherwise, where the flat image is 4-way."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("lds_layout_model", ROOT / "tools" / "exp" / "lds_layout_model.py")
model = importlib.util.module_from_spec(spec)
spec.loader.exec_module(model)

CHANNELS = (1, 2, 3, 6, 8, 32, 64)
MIS = (0, 1, 3, 8)
# format -> per channel count of CHANNELS: ((write, write with bytes apart) at address mod 16 == 0, the same at 1, 3 and 8)
A, B, C3 = ((1, 1), (2, 2)), ((2, 2), (2, 2)), ((3, 3), (3, 3))
WRITE = {"u8": (((1, 4), (1, 4)), ((1, 2), (1, 2)), ((1, 2), (1, 2)), B, A, A, A),
         "s16": (((1, 2), (1, 2)), A, B, C3, A, A, A),
         "s24": (((1, 2), (1, 2)), B, C3, C3, B, B, B),
         "s32": (A, A, C3, B, A, A, A),
         "f32": (A, A, C3, B, A, A, A),
         "f64": (A, A, B, C3, A, A, A)}
FLAT_WRITE = {"u8": (1, 1, 1, 2, 2, 8, 16), "s16": (1, 1, 2, 1, 4, 16, 32), "s24": (1, 2, 2, 2, 2, 8, 16), "s32": (1, 2, 1, 2, 8, 32, 32),
              "f32": (1, 2, 1, 2, 8, 32, 32), "f64": (2, 4, 2, 4, 16, 32, 32)}


def test_the_model_exposes_the_issue_grid():
    assert model.PCMENC_CHANNELS == CHANNELS and model.PCMENC_MIS == MIS and sorted(WRITE) == sorted(model.PCM_WIDTH)


@pytest.mark.parametrize("fmt", list(WRITE))
def test_degrees_of_the_committed_layout(fmt):
    for channels, quoted in zip(CHANNELS, WRITE[fmt]):
        for mis in MIS:
            res = model.pcm_encode(fmt, channels, mis)
            print(fmt, channels, mis, res)
            assert (res["encode write"], res["encode write, bytes apart"]) == quoted[mis != 0], (fmt, channels, mis, res)
            assert res["drain read"] == (1 if mis == 0 else 2), (fmt, channels, mis, res)
            assert res["encode write"] <= 3


@pytest.mark.parametrize("fmt", list(WRITE))
def test_the_flat_image_is_what_the_pads_replace(fmt):
    for channels, quoted in zip(CHANNELS, FLAT_WRITE[fmt]):
        flat = model.pcm_encode(fmt, channels, 0, phys=model.pcm_flat)
        assert flat["encode write"] == quoted and flat["drain read"] == 4, (fmt, channels, flat)


def test_byte_model_of_sub_dword_stores():
    assert model._degree_by_byte("write_b32", [l for l in range(64)]) == 4            # four lanes per dword, every byte its own access
    assert model.degree("write_b32", [l & ~3 for l in range(64)]) == 1                # the same lanes with a dword as one address
    assert model._degree_by_byte("write_b32", [128 * l for l in range(64)]) == 32


def test_source_and_model_agree():
    """the layout function, the tile budget, the widths and the image's size in pcmenc.hip are the model's, and the layout is
    pcm.hip's: a changed layout must change the model"""
    src = (ROOT / "friture_amd" / "csrc" / "pcmenc.hip").read_text()
    assert "pcmenc_phys(unsigned D) { return D + (D >> 5) + (D >> 10); }" in src
    assert "kTileBytes = 32768;" in src and "kTileBytes / (channels * W) / 64 * 64" in src
    assert "kWidth[kFormats] = {1, 2, 3, 4, 4, 8}" in src
    assert "kLdsDwords = pcmenc_phys((15 + kTileBytes) / 4 + 1) + 1" in src
    assert "kThreads = 256" in src
    assert [model.pcm_phys(D) for D in (31, 32, 1024)] == [31, 33, 1057]
    # the last byte of a full tile at the largest misalignment lies inside the array
    assert model.pcm_phys((15 + model.PCM_TILE_BYTES - 1) // 4) < model.pcm_phys((15 + model.PCM_TILE_BYTES) // 4 + 1) + 1
    from friture_amd import _lib
    lib = _lib.load()
    for code, (fmt, w) in enumerate(model.PCM_WIDTH.items()):
        for channels in CHANNELS:
            F = lib.frt_pcm_tile_frames(code, channels)
            assert F == model.pcm_tile_frames(fmt, channels) == model.PCM_TILE_BYTES // (channels * w) // 64 * 64
