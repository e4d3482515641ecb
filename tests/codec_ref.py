"""Plain references for the bitstream kernels of masic_amd/csrc/codec.hip and the coder of rans.hip: numpy and Python integers only,
no GPU and no ctypes.  Shared by tests/test_cpu_codec_ref.py and tests/test_gpu_codec_edges.py.

  table_counts_f64   the coding-table recipe of the reference (MASIC.py:1004-1043) in float64, vectorised over rows;
  table_counts_f32   the same recipe in numpy float32 in the operation order of gmm_cdf_kernel: a CPU stand-in to see whether float32
                     arithmetic alone moves a count of some input by 1 or more (it chooses inputs, it is never a reference);
  rans_decode_py     a decoder for one channel stream, from the format described in codec.hip / rans.hip;
  ideal_bits         the code length the tables themselves assign to a symbol sequence;
  code_length_slack  the bound a channel stream's length must satisfy, and how much room is left under it."""
import bisect

import numpy as np
from scipy.special import erfc

TOTAL = 1 << 16


def table_counts_f64(sigma, mu, logits, minmax, bound):
    """sigma, mu, logits: [rows][K] -> (rounded counts [rows][L], the unrounded float64 values [rows][L]), L = 2 * minmax + 1:
    softmax over K, |s - (mu + minmax)|, the two 0.5 * erfc cumulatives, clip to [2^-16, 1], renormalise to 2^16, round."""
    sigma, mu, logits = (np.asarray(a, dtype=np.float64).reshape(len(a), -1) for a in (sigma, mu, logits))
    w = np.exp(logits - logits.max(axis=1, keepdims=True))
    w = w / w.sum(axis=1, keepdims=True)
    s = np.arange(2 * minmax + 1, dtype=np.float64)
    sc = np.maximum(sigma, bound)
    pmf = np.zeros((sigma.shape[0], s.size))
    phi = lambda t: 0.5 * erfc(-(2 ** -0.5) * t)
    for k in range(sigma.shape[1]):
        v = np.abs(s[None, :] - (mu[:, k, None] + minmax))
        pmf += (phi((0.5 - v) / sc[:, k, None]) - phi((-0.5 - v) / sc[:, k, None])) * w[:, k, None]
    clip = np.clip(pmf, 1.0 / TOTAL, 1.0)
    raw = clip / clip.sum(axis=1, keepdims=True) * TOTAL
    return np.round(raw), raw


def table_counts_f32(sigma, mu, logits, minmax, bound):
    """The kernel's arithmetic in numpy float32 -> (counts after the total is forced to 2^16 at the mode [rows][L] int64, the
    unrounded float32 values [rows][L]).  Lanes own runs of ceil(L / 64) entries, partial sums go through the xor butterfly."""
    f = np.float32
    sigma, mu, logits = (np.asarray(a, dtype=f).reshape(len(a), -1) for a in (sigma, mu, logits))
    R, K = sigma.shape
    L = 2 * minmax + 1
    w = np.exp(logits - logits.max(axis=1, keepdims=True)).astype(f)
    ws = np.zeros(R, dtype=f)
    for k in range(K):
        ws = ws + w[:, k]
    w = w / ws[:, None]
    sk = np.maximum(sigma, f(bound))
    mk = mu + f(minmax)
    s = np.arange(L, dtype=f)
    cst = f(-0.70710678118654752440)
    pm = np.zeros((R, L), dtype=f)
    for k in range(K):
        v = np.abs(s[None, :] - mk[:, k, None])
        up = f(0.5) * erfc(cst * ((f(0.5) - v) / sk[:, k, None])).astype(f)
        lo = f(0.5) * erfc(cst * ((f(-0.5) - v) / sk[:, k, None])).astype(f)
        term = (up - lo) * w[:, k, None]
        pm = term if k == 0 else pm + term
    pm = np.minimum(np.maximum(pm, f(1.0 / TOTAL)), f(1.0))
    chunk = (L + 63) // 64
    part = np.zeros((R, 64), dtype=f)
    for j in range(chunk):                                   # lane l adds its entries l * chunk + j in order
        idx = np.arange(64) * chunk + j
        ok = idx < L
        part[:, ok] = part[:, ok] + pm[:, idx[ok]]
    o = 32
    while o:
        part = part + part[:, np.arange(64) ^ o]
        o >>= 1
    raw = pm / part[:, :1] * f(TOTAL)
    cnt = np.maximum(np.rint(raw), 1).astype(np.int64)
    mode = cnt.argmax(axis=1)                                # largest count, first index
    cnt[np.arange(R), mode] += TOTAL - cnt.sum(axis=1)
    return cnt, raw


def rans_decode_py(stream_bytes, starts_rows):
    """One channel stream (little-endian u32 words; the state starts as w0 | w1 << 32, the next word is word 2) against one row of
    interval starts per symbol (starts[0] = 0, strictly increasing, the last interval ends at 2^16) -> (symbols, finished): finished
    says that every word was consumed and the state ended at 2^31, where every encoder starts."""
    data = bytes(stream_bytes)
    if len(data) < 8 or len(data) % 4:
        raise ValueError("a stream is at least two whole words")
    words = [int.from_bytes(data[i:i + 4], "little") for i in range(0, len(data), 4)]
    x, pos, out = words[0] | (words[1] << 32), 2, []
    for row in starts_rows:
        row = [int(v) for v in row]
        cum = x & 0xFFFF
        s = bisect.bisect_right(row, cum) - 1                # the last entry with start <= cum
        if s < 0:
            raise ValueError("a table does not start at 0")
        start = row[s]
        freq = (row[s + 1] if s + 1 < len(row) else TOTAL) - start
        x = freq * (x >> 16) + cum - start
        if x < (1 << 31):
            if pos >= len(words):
                raise ValueError("the stream ends before its last symbol")
            x = (x << 32) | words[pos]
            pos += 1
        out.append(s)
    return out, pos == len(words) and x == (1 << 31)


def ideal_bits(freqs):
    """sum of -log2(f / 2^16) over the coded symbols' frequencies, float64"""
    return float(-np.log2(np.asarray(freqs, dtype=np.float64) / TOTAL).sum())


def code_length_slack(nbytes, freqs):
    """The length of one channel stream against what its own tables say: ideal - 1 <= 8 * nbytes <= ideal + 96 + 1e-4 * n.
    (The coder's 64-bit state holds at least 31 bits and is flushed whole: at most 64 + 32 bits beyond the payload, words of 32 bits;
    a coding step with x >= 2^31 and a 2^16 total loses less than log2(1 + 2^-15) < 1e-4 bits.)
    -> (bits above the lower bound, bits left under the upper bound); both are >= 0 when the bound holds."""
    ideal, n = ideal_bits(freqs), np.asarray(freqs).size
    return 8 * nbytes - (ideal - 1), ideal + 96 + 1e-4 * n - 8 * nbytes


def edge_tables(rs, nrows, L, kind="edge"):
    """Frequencies [nrows][L] of strictly increasing tables with a 2^16 total.  "edge": one symbol at a random place holds
    65536 - (L - 1), every other one has freq == 1; "random": small random counts with several freq == 1 symbols, the rest of the
    total on one symbol."""
    if kind == "edge":
        f = np.ones((nrows, L), dtype=np.int64)
    else:
        f = rs.randint(1, max(2, min(60, (TOTAL - L) // L)), size=(nrows, L)).astype(np.int64)
        ones = rs.rand(nrows, L) < 0.25
        ones[:, [0, L - 1]] = rs.rand(nrows, 2) < 0.5
        f[ones] = 1
    big = rs.randint(L, size=nrows)
    f[np.arange(nrows), (big + 1 + rs.randint(L - 1, size=nrows)) % L] = 1    # at least one freq == 1 symbol in every row
    f[np.arange(nrows), big] = 1
    f[np.arange(nrows), big] = TOTAL - (f.sum(axis=1) - 1)
    assert f.min() >= 1 and (f.sum(axis=1) == TOTAL).all()
    return f


def starts_of(freqs):
    """interval starts [rows][L] (int64) of frequencies [rows][L]"""
    f = np.asarray(freqs, dtype=np.int64)
    return np.concatenate([np.zeros((f.shape[0], 1), dtype=np.int64), np.cumsum(f, axis=1)[:, :-1]], axis=1)


def check_counts(freq, want, raw):
    """The condition on a kernel's counts `freq` [rows][L] against table_counts_f64's (want, raw): every entry except at most one per
    row lies within 1 of max(want, 1); the exception -- the mode, which absorbs the forcing of the total to 2^16 -- is an entry whose
    float64 count is within 1 of the row's largest, and holds 2^16 minus the row's other entries.  -> (the largest deviation outside
    the exceptions, the largest deviation of an exception).  AssertionError names the first row that leaves the condition."""
    freq = np.asarray(freq, dtype=np.int64)
    d = np.abs(freq - np.maximum(want, 1))
    worst, worst_mode = 0, 0
    for r in range(freq.shape[0]):
        out = np.flatnonzero(d[r] > 1)
        assert out.size <= 1, (r, out.tolist(), d[r, out].tolist())
        if out.size:
            e = int(out[0])
            assert raw[r, e] >= raw[r].max() - 1, (r, e, float(raw[r, e]), float(raw[r].max()))
            assert freq[r, e] == TOTAL - (freq[r].sum() - freq[r, e]), (r, e)
            worst_mode = max(worst_mode, int(d[r, e]))
            worst = max(worst, int(np.delete(d[r], e).max()))
        else:
            worst = max(worst, int(d[r].max()))
    return worst, worst_mode


REGIMES = ("sharp", "flat", "logits", "mode", "random")


def regime_params(regime, n, K, minmax, rs):
    """Entropy parameters (sigma, mu, logits), float32 [n][K], of n table rows in one of the regimes the table kernel is tested in; the
    variants of a regime cycle with the row index.
      sharp   sigma in {0, 0.05, 0.11} (at or under the scale bound 0.11), mu on integers, on exact half-integers, and outside the
              alphabet by +-(minmax + 20);
      flat    sigma in {50, 1e3, 1e6}: every count is about 65536 / L;
      logits  all equal / spread over +-60 / one at +200 (the other weights underflow to exactly 0);
      mode    a sharp mode on symbol 0, on L - 1, on the last entry of one lane's run, on the first of the next lane's, and halfway
              between those two (two equal largest counts: the mode reduction must take the first);
      random  sigma in [0, 6], |mu| <= 0.8 minmax, logits ~ 2 N(0, 1).
    Two choices keep float32 arithmetic ALONE (table_counts_f32 against table_counts_f64, tests/test_cpu_codec_ref.py) within one
    count, the condition the kernel is held to:
      * every mu is a multiple of 1/256, so that mu + minmax is exact in float32.  Rounding that sum (half an ulp of 512 is 3e-5) moves
        the count next to a sharp mode by 65536 * pdf / sigma * 3e-5, about 7 counts at sigma = 0.11 and minmax = 511;
      * a flat row has the same sigma in all K components.  At sigma = 1e3 both cumulatives are 0.5 within 3e-4 and their difference
        keeps 1e-4 of relative precision; mixed with a sigma = 50 component of small weight that is an absolute error of more than one
        count.  (For the same reason the flat regime is not run below minmax = 5: at L = 3 the same 1e-4 is 3 counts.)"""
    L = 2 * minmax + 1
    r = np.arange(n)
    sigma = rs.uniform(0.0, 6.0, (n, K))
    mu = np.round(rs.uniform(-0.8 * minmax, 0.8 * minmax, (n, K)) * 256) / 256      # mu + minmax is exact in float32 (see below)
    logits = rs.standard_normal((n, K)) * 2
    if regime == "sharp":
        sigma = np.array([0.0, 0.05, 0.11])[(r[:, None] + rs.randint(3, size=(n, K)) * (np.arange(K) > 0)) % 3]
        kind = (r[:, None] // 3 + rs.randint(4, size=(n, K)) * (np.arange(K) > 0)) % 4
        whole = rs.randint(-minmax, minmax + 1, size=(n, K)).astype(np.float64)
        half = rs.randint(-minmax, minmax, size=(n, K)) + 0.5
        mu = np.choose(kind, [whole, half, np.full((n, K), minmax + 20.0), np.full((n, K), -(minmax + 20.0))])
    elif regime == "flat":
        sigma = np.repeat(np.array([50.0, 1e3, 1e6])[r % 3][:, None], K, axis=1)       # one sigma per row (see below)
    elif regime == "logits":
        v = r % 3
        logits[v == 0] = rs.uniform(-5, 5, (int((v == 0).sum()), 1))
        spread = np.linspace(-60.0, 60.0, K) if K > 1 else np.array([60.0])
        logits[v == 1] = np.stack([rs.permutation(spread) for _ in range(int((v == 1).sum()))])
        logits[r[v == 2], rs.randint(K, size=int((v == 2).sum()))] = 200.0
    elif regime == "mode":
        chunk = (L + 63) // 64
        lane = rs.randint(0, (L - 1) // chunk, size=n)                        # lanes whose run is followed by another entry
        last = (lane + 1) * chunk - 1                                          # the last entry of the lane's run; last + 1 < L
        assert (last + 1 < L).all()
        at = np.choose(r % 5, [np.zeros(n), np.full(n, L - 1.0), last, last + 1.0, last + 0.5])
        mu = np.repeat((at - minmax)[:, None], K, axis=1)
        sigma = rs.uniform(0.05, 0.6, (n, K))
    elif regime != "random":
        raise ValueError(regime)
    return sigma.astype(np.float32), mu.astype(np.float32), logits.astype(np.float32)
