"""The shuffled stream of the ray bank restated in numpy integers (csrc/mnrf_bank.hip states the contract in its header
comment; this file restates it, the tests hold the two equal).

N = slots * H * W < 2^32.  Lane l of rank r in a world of w at step s takes stream position p = (s * w + r) * B + l;
epoch = p // N, i = p % N, g = perm(seed, epoch)(i).  perm is a balanced Feistel network with cycle walking:
  half  = ceil(max(2, bit_length(N - 1)) / 2), mask = 2^half - 1
  mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (all modulo 2^32)
  key_r = mix32(mix32(mix32(mix32(seed_lo + 0x9e3779b9 * (r + 1)) ^ seed_hi) ^ epoch_lo) ^ epoch_hi),  r = 0 .. ROUNDS - 1
  one pass over x: (L, R) = (x >> half, x & mask); ROUNDS rounds (L, R) <- (R, L ^ (mix32(R ^ key_r) & mask)); x = L << half | R
  perm(i): x = i; pass; while x >= N: pass
Everything is vectorised over numpy uint64 arrays holding 32-bit values (masked after every multiply)."""
import numpy as np

ROUNDS = 6
_M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def half_bits(n):
    return (max(2, int(n - 1).bit_length()) + 1) // 2


def round_keys(seed, epoch, rounds=ROUNDS):
    """(rounds, len(epoch)) uint64 array of 32-bit keys; epoch: array of non-negative integers below 2^64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    epoch = np.atleast_1d(np.asarray(epoch, np.uint64))
    lo, hi = epoch & _M32, epoch >> np.uint64(32)
    keys = []
    for r in range(rounds):
        k = mix32(np.uint64(((seed & 0xFFFFFFFF) + 0x9E3779B9 * (r + 1)) & 0xFFFFFFFF))
        k = mix32(k ^ np.uint64(seed >> 32))
        keys.append(mix32(mix32(k ^ lo) ^ hi))
    return np.stack(keys)


def perm(i, n, seed, epoch, rounds=ROUNDS, return_walks=False):
    """perm(seed, epoch)(i) elementwise; i and epoch broadcast to one shape.  return_walks: also the largest number of passes."""
    i, epoch = np.broadcast_arrays(np.atleast_1d(np.asarray(i, np.uint64)), np.atleast_1d(np.asarray(epoch, np.uint64)))
    assert 1 <= n < 2 ** 32 and (i < np.uint64(n)).all()
    half = np.uint64(half_bits(n))
    mask = np.uint64((1 << int(half)) - 1)
    keys = round_keys(seed, epoch.reshape(-1), rounds).reshape((rounds,) + i.shape)
    x = i.copy()
    todo = np.ones(x.shape, bool)
    walks = 0
    while todo.any():
        walks += 1
        xs = x[todo]
        L, R = xs >> half, xs & mask
        for r in range(rounds):
            L, R = R, L ^ (mix32(R ^ keys[r][todo]) & mask)
        x[todo] = (L << half) | R
        todo = x >= np.uint64(n)
    return (x.astype(np.int64), walks) if return_walks else x.astype(np.int64)


def positions(step, batch, rank=0, world=1):
    """Stream positions of the lanes of one step, as Python-exact uint64."""
    base = (int(step) * int(world) + int(rank)) * int(batch)
    return np.array([(base + l) & 0xFFFFFFFFFFFFFFFF for l in range(batch)], np.uint64)


def stream(p, n, seed, rounds=ROUNDS):
    """The global ray indices at stream positions p."""
    p = np.asarray(p, np.uint64)
    epoch = p // np.uint64(n)
    return perm(p - epoch * np.uint64(n), n, seed, epoch, rounds)


def draw_indices(n, step, batch, seed, rank=0, world=1):
    return stream(positions(step, batch, rank, world), n, seed)
