"""attn_res = 32 (gen_block_32 with the reference's AttentionBlock) in the layout and the step configuration; no GPU.
The default stays the parent's layout for every resolution."""
import pytest

from moegan_mi import layout
from moegan_mi.layout import attn_res_of, gen_blocks, generator_shapes, max_res_of


@pytest.mark.parametrize("R", layout.MAX_RESOLUTIONS)
@pytest.mark.parametrize("E", [4, 8])
def test_default_shapes_unchanged(E, R):
    a, b = generator_shapes(E, R), generator_shapes(E, R, attn_res=16)
    assert list(a.items()) == list(b.items())
    assert not any(k.startswith("gen_block_32.attn_block.") for k in a)
    assert attn_res_of(a) == 16 and max_res_of(a) == R
    assert [blk[5] for blk in gen_blocks(R)] == [True] * 3 + [False] * (len(gen_blocks(R)) - 3)


@pytest.mark.parametrize("R", [32, 64, 128])
def test_attn32_shapes_and_order(R):
    E = 4
    base, d = generator_shapes(E, R), generator_shapes(E, R, attn_res=32)
    keys = list(d)
    new = [k for k in keys if k not in base]
    assert new and all(k.startswith("gen_block_32.attn_block.") for k in new)
    assert [k for k in keys if k in base] == list(base)  # the other keys keep their order ...
    assert all(d[k] == base[k] for k in base)  # ... and shapes
    # directly after the block's conv_block.* keys, as one contiguous run
    i0 = keys.index(new[0])
    assert keys[i0 - 1].startswith("gen_block_32.conv_block.") and keys[i0:i0 + len(new)] == new
    nxt = keys[i0 + len(new)]
    assert nxt.startswith("gen_block_64.conv_block.") if R >= 64 else nxt.startswith("to_rgb_8.")
    # the keys and shapes of the 16x16 block's AttentionBlock (same C = 128), in its order
    ref16 = [(k[len("gen_block_16"):], v) for k, v in base.items() if k.startswith("gen_block_16.attn_block.")]
    assert [(k[len("gen_block_32"):], d[k]) for k in new] == ref16
    r = "gen_block_32.attn_block.moe.router."
    assert (d[r + "epsilon_f"], d[r + "epsilon_t"], d[r + "epsilon_c"]) == ((128, 128), (512, 128), (256, E))
    assert not any("gen_block_32.conv_block." in k and "offset_net" in k for k in keys)  # no offset head above 16
    assert attn_res_of(d) == 32 and max_res_of(d) == R
    assert [b[0] for b in gen_blocks(R, 32) if b[5]] == ["gen_block_4", "gen_block_8", "gen_block_16", "gen_block_32"]


def test_attn_res_validation():
    with pytest.raises(ValueError, match="attn_resolution"):
        gen_blocks(16, 32)
    with pytest.raises(ValueError, match="attn_resolution"):
        gen_blocks(64, 64)
    with pytest.raises(ValueError, match="attn_resolution"):
        generator_shapes(4, 32, attn_res=8)
    from moegan_mi.step import StepConfig
    assert StepConfig().attn_res == 16 and StepConfig(max_res=64, attn_res=32).attn_res == 32
    with pytest.raises(ValueError, match="attn_resolution 32 needs max_resolution >= 32"):
        StepConfig(max_res=16, attn_res=32)
    with pytest.raises(ValueError, match="attn_resolution must be one of"):
        StepConfig(max_res=64, attn_res=64)
