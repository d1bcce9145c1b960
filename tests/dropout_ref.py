"""numpy restatement of the dropout mask (include/mantle_hip.h, mc_dropout): Philox4x32-10 (Salmon et al., SC 2011) and
the mapping from (seed, step, layer, logical element) to keep flags.  Written from the definition, independent of
csrc/philox.h, so that the tests compare two implementations."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key, rounds=10):
    """ctr: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def keep16(p):
    """T = clamp(round((1 - p) 65536), 1, 65535)."""
    return min(max(int(round((1.0 - p) * 65536.0)), 1), 65535)


def scale(p):
    """s = f32(65536 / T)."""
    return np.float32(65536.0 / keep16(p))


def keep_vectors(seed, step, layer, first_vec, n_vec, T):
    """[n_vec, 8] bool: keep flags of the 8 channels of the CB8 vectors first_vec .. first_vec + n_vec - 1.
    seed: (seed_lo, seed_hi)."""
    v = np.uint64(first_vec) + np.arange(n_vec, dtype=np.uint64)
    out = philox4x32([v & MASK32, v >> np.uint64(32), np.uint32(layer), np.uint32(step)], seed)
    f = np.empty((n_vec, 8), np.uint32)
    for j in range(8):
        f[:, j] = (out[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
    return f < np.uint32(T)


def keep_nchw(seed, step, layer, N, C, H, W, T):
    """[N, C, H, W] bool keep mask of a tensor stored as CB8 [N][C8][H][W][8]: vector v = ((n C8 + cb) H + y) W + x."""
    C8 = (C + 7) // 8
    k = keep_vectors(seed, step, layer, 0, N * C8 * H * W, T).reshape(N, C8, H, W, 8)
    return np.ascontiguousarray(k.transpose(0, 1, 4, 2, 3).reshape(N, C8 * 8, H, W)[:, :C])
