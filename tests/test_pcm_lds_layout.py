"""The LDS image of pcm_decode_kernel (csrc/pcm.hip) against the bank rules of gfx950, on the CPU: tools/exp/lds_layout_model.py
restates the layout function the kernel stores and reads through, pcm_phys(D) = D + (D >> 5) + (D >> 10) on logical dwords, and
counts the distinct addresses that meet on one bank per ds_read_b32 / ds_write_b32 lane group.  What DESIGN.md R2 quotes is
asserted here: frames whose size is a power of two (s32 x 32 = 128 B, f64 x 32 = 256 B, ...) read conflict free where the flat
image would serialise a whole lane group, the fill, which the compiler emits as ds_write2_b32 pairs, is conflict free with the dwords of a pair as accesses of their own and 2-way —
the floor of its 16-byte lane stride — with them together, and no shape of the table is worse than 3-way."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("lds_layout_model", ROOT / "tools" / "exp" / "lds_layout_model.py")
model = importlib.util.module_from_spec(spec)
spec.loader.exec_module(model)

# (format, channels, address mod 16) -> decode-read degree with the pads, as DESIGN.md R2 lists them
QUOTED = {("s16", 2, 0): 1, ("s24", 2, 0): 2, ("s24", 8, 0): 2, ("s32", 32, 0): 1, ("f64", 32, 0): 1, ("s32", 16, 0): 1, ("f64", 16, 0): 1,
          ("s32", 64, 0): 1, ("f64", 64, 0): 1, ("f64", 1, 0): 1, ("s24", 6, 0): 3, ("s32", 32, 2): 2, ("f64", 32, 4): 2, ("s16", 2, 1): 2}
FLAT = {("s32", 32, 0): 32, ("f64", 32, 0): 32, ("s32", 16, 0): 16, ("f64", 16, 0): 32, ("f64", 1, 0): 2, ("s16", 2, 0): 1}


def test_bank_model_of_the_dword_accesses():
    assert model.degree("read_b32", [4 * l for l in range(64)]) == 1
    assert model.degree("read_b32", [128 * l for l in range(64)]) == 32          # a 128-byte lane stride: one bank
    assert model.degree("read_b32", [64 * l for l in range(64)]) == 16
    assert model.degree("read_b32", [l // 4 * 4 for l in range(64)]) == 1          # four lanes in one dword broadcast
    assert model.degree("write_b32", [16 * l for l in range(64)]) == 4
    assert model.degree("write2_b32", [(8 * l, 8 * l + 4) for l in range(64)]) == 1           # 16 lanes x 2 dwords: every bank once
    assert model.degree("write2_b32", [(16 * l, 16 * l + 4) for l in range(64)]) == 2


def test_layout_function_is_a_padding():
    """Monotonic, so injective; the four dwords of a 16-byte granule stay adjacent; the image of a full tile at the largest
    misalignment, with the two dwords an unaligned sample reads past it, fits the kernel's array."""
    phys = [model.pcm_phys(D) for D in range(8300)]
    assert all(b > a for a, b in zip(phys, phys[1:]))
    assert all(model.pcm_phys(D + i) == model.pcm_phys(D) + i for D in range(0, 8296, 4) for i in range(4))
    assert model.pcm_phys(31) == 31 and model.pcm_phys(32) == 33 and model.pcm_phys(1024) == 1024 + 32 + 1
    last = (15 + model.PCM_TILE_BYTES - 1) // 4 + 2                                  # the third dword of a misaligned last f64
    assert model.pcm_phys(last) < model.pcm_phys((15 + model.PCM_TILE_BYTES + 8) // 4 + 1) + 1


@pytest.mark.parametrize("case", sorted(QUOTED), ids=lambda c: f"{c[0]}x{c[1]}@{c[2]}")
def test_decode_read_degrees_are_the_quoted_ones(case):
    res = model.pcm_decode(*case)
    print(case, res)
    assert res["decode read"] == QUOTED[case]
    assert res["fill write"] == 1                            # the dwords of the emitted ds_write2_b32 as accesses of their own
    assert res["fill write, pairs together"] == 2            # or together, in ds_write_b64's groups: the floor of a 16-byte lane stride
    assert model.pcm_decode(*case, phys=model.pcm_flat)["fill write, pairs together"] == 2


@pytest.mark.parametrize("case", sorted(FLAT), ids=lambda c: f"{c[0]}x{c[1]}@{c[2]}")
def test_the_flat_image_is_what_the_pads_replaced(case):
    assert model.pcm_decode(*case, phys=model.pcm_flat)["decode read"] == FLAT[case]


def test_no_listed_shape_is_worse_than_three_way():
    for case in model.PCM_CASES:
        res = model.pcm_decode(*case)
        assert res["decode read"] <= 3 and res["fill write"] == 1, (case, res)


def test_source_and_model_agree():
    """the layout function, the tile budget and the tile rule of the model are the kernel's (a changed layout must change the model)"""
    src = (ROOT / "friture_amd" / "csrc" / "pcm.hip").read_text()
    assert "pcm_phys(unsigned D) { return D + (D >> 5) + (D >> 10); }" in src
    assert "kTileBytes = 32768;" in src and "kTileBytes / (channels * kWidth[format]) / 64 * 64" in src
    assert "kWidth[kFormats] = {1, 2, 3, 4, 4, 8}" in src
    assert "kLdsDwords = pcm_phys((15 + kTileBytes + 8) / 4 + 1) + 1" in src
    from friture_amd import _lib
    lib = _lib.load()
    for code, (fmt, w) in enumerate(model.PCM_WIDTH.items()):
        for channels in (1, 2, 3, 6, 8, 32, 64):
            assert lib.frt_pcm_tile_frames(code, channels) == model.pcm_tile_frames(fmt, channels)
