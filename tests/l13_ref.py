"""numpy encoder / decoder of the lossless 13-bit weight image, written from the description in include/ua2hip.h
(ua2_pack_linear_l13).  Input and output are the PACKED bf16 form of a weight as uint16: [tiles][chunks][64 lanes][8 elements]."""
import numpy as np

GROUP_BYTES = 3328


def tile_base(packed):
    """base byte of every tile: max(largest E[7:1] - 15, 0)."""
    e7 = (packed >> 8) & 0x7f
    return np.maximum(e7.reshape(packed.shape[0], -1).max(axis=1).astype(np.int32) - 15, 0).astype(np.uint8)


def encode(packed):
    """packed: uint16 [T, C, 64, 8], C % 4 == 0 -> (image uint8 [T * C / 4 * 3328], base uint8 [T], escapes int)."""
    T, C, L, E = packed.shape
    assert L == 64 and E == 8 and C % 4 == 0
    base = tile_base(packed)
    b = base.astype(np.int32)[:, None, None, None]
    e7 = ((packed >> 8) & 0x7f).astype(np.int32)
    escapes = int(((e7 != 0) & (e7 <= b)).sum())
    q = np.clip(e7 - b, 0, 15).astype(np.uint32)                  # 0: E[7:1] == 0 (and, in an unusable image, an escape)
    low = (packed & 0xff).astype(np.uint8)
    sign = (packed >> 15).astype(np.uint32)
    G = C // 4
    img = np.zeros((T, G, GROUP_BYTES), dtype=np.uint8)
    lowg = low.reshape(T, G, 2, 2, 64, 8)                          # [tile, group, pair, chunk of the pair, lane, element]
    # low bytes: pair p = [64 lanes][16 B] = the lane's 8 of chunk 2p, then its 8 of chunk 2p + 1
    img[:, :, :2048] = lowg.transpose(0, 1, 2, 4, 3, 5).reshape(T, G, 2048)
    # codes: [64 lanes][4 chunks] dwords, byte b = q(element b) | q(element b + 4) << 4
    qg = q.reshape(T, G, 4, 64, 8)
    code = (qg[..., :4] | (qg[..., 4:] << 4)).astype(np.uint8)     # [T, G, chunk, lane, byte]
    img[:, :, 2048:3072] = code.transpose(0, 1, 3, 2, 4).reshape(T, G, 1024)
    # signs: [64 lanes] dwords, bit 8 b + 2 c + h = sign of element 4 h + b of chunk c
    sg = sign.reshape(T, G, 4, 64, 2, 4)                           # [T, G, c, lane, h, b]
    word = np.zeros((T, G, 64), dtype=np.uint32)
    for c in range(4):
        for h in range(2):
            for bb in range(4):
                word |= sg[:, :, c, :, h, bb] << np.uint32(8 * bb + 2 * c + h)
    img[:, :, 3072:] = word.astype("<u4").view(np.uint8).reshape(T, G, 256)
    return img.reshape(-1), base, escapes


def decode(image, base, T, C):
    """inverse of encode for an escape-free image: uint16 [T, C, 64, 8]."""
    G = C // 4
    img = image.reshape(T, G, GROUP_BYTES)
    low = img[:, :, :2048].reshape(T, G, 2, 64, 2, 8).transpose(0, 1, 2, 4, 3, 5).reshape(T, C, 64, 8).astype(np.uint16)
    code = img[:, :, 2048:3072].reshape(T, G, 64, 4, 4).transpose(0, 1, 3, 2, 4).astype(np.uint16)   # [T, G, chunk, lane, byte]
    q = np.concatenate([code & 0xf, code >> 4], axis=-1).reshape(T, C, 64, 8)
    word = img[:, :, 3072:].copy().view("<u4").reshape(T, G, 64)
    sign = np.zeros((T, G, 4, 64, 2, 4), dtype=np.uint16)
    for c in range(4):
        for h in range(2):
            for bb in range(4):
                sign[:, :, c, :, h, bb] = (word >> np.uint32(8 * bb + 2 * c + h)) & 1
    sign = sign.reshape(T, C, 64, 8)
    b = base.astype(np.uint16)[:, None, None, None]
    e7 = np.where(q != 0, q + b, 0).astype(np.uint16)
    return ((sign << 15) | (e7 << 8) | low).astype(np.uint16)
