"""The lossless 13-bit weight image (include/ua2hip.h ua2_pack_linear_l13) as a format: a numpy encoder and decoder written from the
header's description give back every bf16 bit pattern placed in a tile whose window holds it, and report what the window cannot hold."""
import numpy as np

from l13_ref import GROUP_BYTES, decode, encode, tile_base

C = 4                 # chunks per tile: one group
PER_TILE = C * 64 * 8


def _tiles_for_all_patterns():
    """Every one of the 65 536 bf16 bit patterns, grouped so that each tile's window holds its members: patterns are sorted by E[7:1]
    and cut into bands of 15 pairs; pair 0 (q = 0: +-0, subnormals, the lowest normal binade) is added to every tile."""
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    e7 = (pats >> 8) & 0x7f
    pair0 = pats[e7 == 0]
    tiles = []
    for lo in range(1, 128, 15):                                   # pairs lo .. lo + 14: base = lo - 1, q = 1 .. 15
        band = pats[(e7 >= lo) & (e7 < lo + 15)]
        vals = np.concatenate([band, pair0])
        for i in range(0, len(vals), PER_TILE - 2):
            t = np.zeros(PER_TILE, dtype=np.uint16)
            part = vals[i:i + PER_TILE - 2]
            t[:len(part)] = part
            # pin the window: its top pair and its bottom pair are in every tile of the band (the two edges), both signs
            t[-2] = np.uint16((min(lo + 14, 127) << 8) | 0x8055)
            t[-1] = np.uint16((lo << 8) | 0x00aa)
            tiles.append(t)
    return np.stack(tiles).reshape(-1, C, 64, 8)


def test_every_bf16_pattern_round_trips():
    packed = _tiles_for_all_patterns()
    assert set(np.unique(packed).tolist()) == set(range(65536))
    image, base, escapes = encode(packed)
    assert escapes == 0
    assert image.size == packed.shape[0] * GROUP_BYTES and image.size * 16 == packed.size * 2 * 13
    back = decode(image, base, packed.shape[0], C)
    assert np.array_equal(back, packed)


def test_zero_pair0_and_window_edges():
    t = np.zeros((1, C, 64, 8), dtype=np.uint16)
    top = 0x3c                                                     # E[7:1] of 1.0 .. 4.0 halves: 0x3c80 = 1/64 ... any pair works
    vals = [0x0000, 0x8000,                                        # +0, -0
            0x0001, 0x807f, 0x0080, 0x80ff,                        # pair 0: subnormals and the lowest normal binade, both signs
            (top << 8) | 0x12, 0x8000 | (top << 8) | 0xff,         # the window's top pair
            ((top - 14) << 8) | 0x00, 0x8000 | ((top - 14) << 8) | 0x80]   # ... and its bottom pair (q = 1)
    flat = t.reshape(-1)
    for lane_group in range(0, flat.size, 64):                     # in every lane group of 8 lanes x 8 elements
        flat[lane_group:lane_group + len(vals)] = vals
    image, base, escapes = encode(t)
    assert base.tolist() == [top - 15] and escapes == 0
    assert np.array_equal(decode(image, base, 1, C), t)
    # a tile of small values only: base clamps at 0 and q is E[7:1] itself
    small = np.full((1, C, 64, 8), 0x0312, dtype=np.uint16)
    image, base, escapes = encode(small)
    assert base.tolist() == [0] and escapes == 0 and np.array_equal(decode(image, base, 1, C), small)


def test_one_weight_below_the_window_is_an_escape():
    rng = np.random.default_rng(0)
    top = 0x40
    e7 = rng.integers(top - 14, top + 1, size=(2, C, 64, 8)).astype(np.uint16)
    t = ((rng.integers(0, 2, size=e7.shape).astype(np.uint16) << 15) | (e7 << 8) | rng.integers(0, 256, size=e7.shape).astype(np.uint16))
    t[:, 0, 0, 0] = np.uint16(top << 8)                            # both tiles reach the top pair
    assert encode(t)[2] == 0
    t[1, 2, 17, 5] = np.uint16(((top - 15) << 8) | 0x33)           # one pair below the window of tile 1
    image, base, escapes = encode(t)
    assert tile_base(t).tolist() == [top - 15, top - 15] and escapes == 1
    back = decode(image, base, 2, C)
    assert np.array_equal(back[0], t[0]) and not np.array_equal(back[1], t[1])    # the image of the escaped tile is not exact: never used
