"""The exchange layout of the one-wavefront M = 512 transform (stft_kernel, N = 1024; fft_core.h LdsXorWave512) against the
bank rules of gfx950, on the CPU: point x lies in slot x ^ ((x >> 3) & 15).  tools/exp/lds_layout_model.py holds the map that
ships and the one it replaced (one pad slot per 8 points), whose gathers are 2-way conflicted — asserted too, so that the model
is seen to tell the two apart."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("lds_layout_model", ROOT / "tools" / "exp" / "lds_layout_model.py")
model = importlib.util.module_from_spec(spec)
spec.loader.exec_module(model)

PATTERNS = {  # lane i, slot s -> point
    "scatter 8i + q": ("write", lambda i, s: 8 * i + s),
    "gather i + 64j": ("read", lambda i, s: i + 64 * s),
    "scatter 64(i>>3) + (i&7) + 8q": ("write", lambda i, s: 64 * (i >> 3) + (i & 7) + 8 * s),
    "second gather i + 64j": ("read", lambda i, s: i + 64 * s),
}


def worst(phys, elem, pattern):
    side, point = PATTERNS[pattern]
    kind = f"{side}_b{8 * elem}"
    return max(model.degree(kind, [elem * phys(point(i, s)) for i in range(64)]) for s in range(8))


@pytest.mark.parametrize("elem", [8, 16])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_shipped_map_is_conflict_free(pattern, elem):
    assert worst(model.wave512_xor, elem, pattern) == 1


def test_shipped_map_is_a_bijection():
    assert sorted(model.wave512_xor(x) for x in range(512)) == list(range(512))


def test_old_map_conflicts_on_the_gathers():
    for pattern in PATTERNS:
        assert worst(model.wave512_pad, 8, pattern) == (2 if "gather" in pattern else 1), pattern


def test_model_entry_matches_the_patterns():
    assert set(model.stft_wave512().values()) == {1}
    assert model.stft_wave512_padded() == {"exchange 1 write": 1, "exchange 1 read": 2, "exchange 2 write": 1, "exchange 2 read": 2}


def _layout_map(src, struct):
    """the expression of `at(int x)` inside `struct NAME { ... }` of fft_core.h, as a Python function of x (C integer operators only)"""
    body = re.search(r"struct\s+" + struct + r"\s*\{(.*?)\n\};", src, re.S).group(1)
    expr = re.search(r"\bat\s*\(\s*int\s+x\s*\)\s*\{\s*return\s+(.*?);", body, re.S).group(1)
    assert re.fullmatch(r"[x0-9\s()^&|+\-*<>a-z_]+", expr), expr
    return lambda x: eval(expr, {"x": x, "lds_pad": model.wave512_pad})


def test_source_and_model_agree_on_the_map():
    """The maps are read out of the source and evaluated, point by point; and stft_kernel gives the swizzle to its N = 1024 register-window
    instances (and only them) as the transform's layout."""
    csrc = ROOT / "friture_amd" / "csrc"
    core = (csrc / "fft_core.h").read_text()
    xor, pad = _layout_map(core, "LdsXorWave512"), _layout_map(core, "LdsPad8")
    assert [xor(x) for x in range(512)] == [model.wave512_xor(x) for x in range(512)]
    assert [pad(x) for x in range(512)] == [model.wave512_pad(x) for x in range(512)]
    flat = re.sub(r"\s+", "", core)
    # the points the passes exchange are the patterns above: thread i scatters base + q p, base = (i - k) 8 + k, k = i mod p (p = 1, 8), and
    # gathers i + j TPF, both through the layout
    assert "constintk=i&(p-1);" in flat and "constintbase=(i-k)*8+k;" in flat
    assert "buf[LAY::at(base+q*p)]=v[q];" in flat and "v[j]=buf[LAY::at(i+j*TPF)];" in flat
    wave = re.sub(r"\s+", "", (csrc / "stft_wave.h").read_text())
    assert "constexprboolXOR_LDS=LOG2M==9&&SHIFT>0;" in wave
    assert "usingLay=std::conditional_t<XOR_LDS,LdsXorWave512,LdsPad8>;" in wave
    assert wave.count("fft_pow2_forward<T,LOG2M,WAVE,Lay>(") == 2 and wave.count("fft_pow2_forward<") == 2
    assert "__shared__Clds[GPB*Lay::size(M)];" in wave and "C*buf=lds+grp*Lay::size(M);" in wave
