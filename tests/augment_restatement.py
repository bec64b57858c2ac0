"""NumPy restatement of lcr_augment_clouds (include/lcr_hip.h, a-1t): Philox4x32-10 in integer arithmetic, the fp32 per-point formula
in the stated order (every operation a separate NumPy call, so each is rounded once), the point-limit selection as a stable argsort
of (word, index), and an fp64 evaluation of the same formula from the same uniforms.  The `plant` arguments introduce one
deliberate mistake each; the GPU test shows that every one of them is seen."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STREAM_NOISE, STREAM_SELECT = 0, 1
U32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10.  counter: four uint32 arrays (or ints) that broadcast, key: two -> uint32 [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                      # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def uniforms(index, sample_id, seed):
    """fp32 [n, 3] uniforms of the noise stream for original indices `index`: (word >> 8) * 2^-24, words 0 .. 2."""
    w = philox4x32((np.asarray(index, np.uint64), 0, int(sample_id), STREAM_NOISE), seed_key(seed))[..., :3]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def select_words(L, sample_id, seed, mask=0xFFFFFFFF):
    w = philox4x32((np.arange(L, dtype=np.uint64), 0, int(sample_id), STREAM_SELECT), seed_key(seed))[..., 0]
    return w & np.uint32(mask)


def select(L, limit, sample_id, seed, mask=0xFFFFFFFF, plant=None):
    """Original indices of the kept points, in output order."""
    if limit is None or limit <= 0 or L <= limit:
        return np.arange(L, dtype=np.int64)
    w = select_words(L, sample_id, seed, mask)
    if plant == "unstable":                            # ties resolved by the LARGER index
        order = np.lexsort((-np.arange(L), w))
    else:
        order = np.argsort(w, kind="stable")
    return order[:limit].astype(np.int64)


def transform_f32(p, u, R, scale, shift, noise, plant=None):
    """The fp32 formula.  p f32 [n,3], u f32 [n,3] uniforms, R [3,3], scale, shift [3], noise — all taken as fp32."""
    f = np.float32
    p, u, R, shift = np.asarray(p, f), np.asarray(u, f), np.asarray(R, f), np.asarray(shift, f)
    scale, noise = f(scale), f(noise)
    if plant == "transposed":
        R = R.T
    c = u if plant == "uncentred" else u - f(0.5)
    n = p + c * noise
    r = np.stack([(R[i, 0] * n[:, 0] + R[i, 1] * n[:, 1]) + R[i, 2] * n[:, 2] for i in range(3)], axis=1)
    if plant == "scaled_shift":
        return r * scale + shift * scale
    return r * scale + shift


def transform_f64(p, u, R, scale, shift, noise):
    """The same formula in fp64 from the same (fp32) inputs and uniforms."""
    d = np.float64
    p, u, R, shift = np.asarray(p, d), np.asarray(u, d), np.asarray(R, d), np.asarray(shift, d)
    n = p + (u - 0.5) * d(noise)
    return (n @ R.T) * d(scale) + shift


def bound(p, scale, shift, noise):
    """7 * 2^-24 * (sqrt(3) * max|p| * max(scale, 1) + |shift|_inf + noise): seven roundings of at most half an ulp of an
    intermediate no larger than that magnitude."""
    mp = float(np.max(np.abs(p))) if len(p) else 0.0
    return 7.0 * 2.0 ** -24 * (np.sqrt(3.0) * mp * max(float(scale), 1.0) + float(np.max(np.abs(shift))) + float(noise))


def augment_cloud(rows, sample_id, R, scale, shift, noise, seed, limit=0, mask=0xFFFFFFFF, plant=None):
    """One cloud: rows f32 [L, C >= 3] -> (out f32 [min(L, limit), 3], kept original indices)."""
    rows = np.asarray(rows, np.float32)
    keep = select(len(rows), limit, sample_id, seed, mask, plant)
    counter = np.arange(len(keep)) if plant == "output_counter" else keep
    u = uniforms(counter, sample_id, seed)
    return transform_f32(rows[keep, :3], u, R, scale, shift, noise, plant), keep


def augment_stack(clouds, sample_ids, Rs, scales, shifts, noises, seed, limit=0, mask=0xFFFFFFFF, plant=None):
    outs = [augment_cloud(c, s, R, sc, sh, nz, seed, limit, mask, plant)[0]
            for c, s, R, sc, sh, nz in zip(clouds, sample_ids, Rs, scales, shifts, noises)]
    return (np.concatenate(outs) if outs else np.zeros((0, 3), np.float32)), [len(o) for o in outs]
