"""Crafted logits rows for the device sampler (csrc/gl3_sample.hip) and a sorted restatement of ToppSampler to aim them with.

The sampler's single-GPU tests draw their rows from random-weight models: near-uniform distributions and coins that land where chance puts
them.  The rows here are built so that a chosen boundary of the kernels is crossed, and every case says which one (its tag) and what must
come out of it (its aim):

  bsm_seqsum_kernel   a chunk of fewer than 1024 elements takes the naive chain, a longer one exact_seqsum_lds; chunks are 4096 elements, so
                      V = 4112 leaves a second chunk of 16; the categorical pick is the strict `coin < cdf` (a coin equal to the cdf at the end
                      of chunk 0 selects the first element of chunk 1), continued from chunk_end[c - 1]; no cdf above the coin: V - 1.
  the radix sort      tiles of 1024: V = 16, 1040, 4112, 9232 leave a last tile with 16 valid elements; btp_scan runs over 256 * tiles entries.
  btp_pick_kernel     works on the candidate count n0, which need not be a multiple of 4: n0 in {1, 2, 3, 5}, on both sides of the naive /
                      exact split (1023 .. 1027) and of the chunk edge (4095 .. 4099, 5123); the truncation rank at rank 0, at the last rank
                      of chunk 0, at the first of chunk 1 and at n0 - 1; a cumulative sum that never exceeds topp (every candidate kept, the
                      reference's lastIndex = 0); coin * cum on rank 0, on the last rank, and one f32 step under the last cdf.
  the tie flag        looks at ranks r - 1 and r + 1: a tie elsewhere in the row stays on the device, a tie at the sampled rank goes to the host.
  values              f32-subnormal and zero probabilities, a probability equal to the cutoff, maxima at the ends, repeated, +0 / -0,
                      temperatures 0.02 and 5.

Nothing here touches the GPU.  Probabilities are oracle_np.softmax's (tests/test_sampler_cases.py holds them equal to the C oracle's, bit
for bit, and proves on the oracle alone that every case hits what its aim says); the expected id of a case is never taken from here but
from oracle_c.sample, the reference's heap.  The sorted restatement (sorted_topp) is used to aim coins and topp values and to predict how
many top-p draws the device answers itself.  ToppSampler's heap emits candidates in non-increasing value order EXCEPT its last three: its
siftDown(indices, 0, i - 1, ..) leaves the last leaf out of every sift, which is harmless while that leaf hangs under a value still in the
heap, but the leaves at heap positions 2 and 1 hang under the root that was just emitted, so the three smallest candidates come out in an
order of the heap's own (sorted_prefix).  While the cumulative sum exceeds topp within the sorted prefix, n0, the truncation rank, the sum
and the sampled RANK are those of a stable descending sort with strictly sequential f32 sums, and only which index stands at a rank shared
by equal values is the heap's business (Sorted.tied).  Otherwise (Sorted.heap_tail: a handful of candidates, or a topp within the last
three candidates' mass of their total, never-exceeded included) nothing but the heap itself says what is drawn; the fields of Sorted then
describe the descending order, which is what the device evaluates before it hands the row to the host."""
import dataclasses
import functools

import numpy as np

from oracle import oracle_np

F32 = np.float32
CHUNK = 4096                 # SM_CHUNK: elements per exact sequential-sum chunk
EXACT_FROM = 1024            # a chunk of at least this many elements (rounded down to a multiple of 4) takes exact_seqsum_lds
RS_TILE = 1024               # elements per radix-sort tile
VOCABS = (16, 1008, 1024, 1040, 4096, 4112, 9232)
COUNTS = (1, 2, 3, 5, 1023, 1024, 1025, 1027, 4095, 4096, 4097, 4099, 5123)
EXTRA_COUNTS = {4112: (4105,)}      # V = 4112: the largest count whose sorted prefix (n0 - 3 ranks) still reaches a few ranks into the second chunk
LOW = F32(-60.0)             # e^-60 = 8.8e-27: a normal f32, 21 orders of magnitude under the smallest cutoff used here
BELOW_ONE = np.nextafter(F32(1.0), F32(0.0))      # the largest rng.nextFloat(1f)
STEP = F32(2.0 ** -12)       # spacing of the candidates' logits: 2000 f32 steps apart as probabilities, exact as logits up to 2^11 * STEP


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def probs_of(logits, temperature):
    """Sampler.java:84-86: divideInPlace(temperature), softmaxInPlace"""
    return oracle_np.softmax((np.asarray(logits, F32) / F32(temperature)).astype(F32))


def is_topp(temperature, topp):
    return temperature > 0 and 0 < topp < 1


def cutoff_of(topp, n):
    """ToppSampler.java:73: (1.0f - topp) / (n - 1), f32 throughout"""
    return F32(F32(F32(1.0) - F32(topp)) / F32(n - 1))


def sorted_candidates(probs, topp):
    """(order, cs): the indices of the candidates (p >= cutoff) in stable descending order of value, and the strictly sequential f32
    cumulative sum of their values in that order"""
    probs = np.asarray(probs, F32)
    cand = np.flatnonzero(probs >= cutoff_of(topp, probs.size))
    order = cand[np.argsort(-probs[cand], kind="stable")]
    return order, np.add.accumulate(probs[order], dtype=F32)


def sorted_prefix(n0):
    """how many of n0 candidates the reference's heap emits in descending order: all but the last three; the first always; two of two"""
    return n0 if n0 <= 2 else max(n0 - 3, 1)


@dataclasses.dataclass(frozen=True)
class Sorted:
    n0: int            # candidates
    last: int          # truncation rank: the first whose cumulative sum exceeds topp, n0 - 1 when none does
    cum: F32           # the cumulative sum at `last`
    exceeded: bool     # whether cum > topp
    rank: int          # the first rank with coin * cum < cdf, `last` when there is none
    fell: bool         # there was none ("in case of rounding errors")
    tied: bool         # another candidate has the value of the sampled rank
    index: int         # the index the stable sort puts at the sampled rank (the token, when the device answers)
    heap_tail: bool    # the sum does not exceed topp within the sorted prefix: the order of the heap's last three decides

    @property
    def host(self):
        """the draw is the host heap's to answer (gl3_get_topp_counts counts it there)"""
        return self.tied or self.heap_tail


def sorted_topp(probs, topp, coin):
    probs = np.asarray(probs, F32)
    order, cs = sorted_candidates(probs, topp)
    n0 = order.size
    over = np.flatnonzero(cs > F32(topp))
    exceeded = over.size > 0
    last = int(over[0]) if exceeded else n0 - 1
    cum = cs[last]
    r = F32(F32(coin) * cum)
    hit = np.flatnonzero(r < cs[:last + 1])
    rank = int(hit[0]) if hit.size else last
    sv = probs[order]
    tied = bool((rank > 0 and sv[rank - 1] == sv[rank]) or (rank + 1 < n0 and sv[rank + 1] == sv[rank]))
    return Sorted(n0, last, cum, bool(exceeded), rank, hit.size == 0, tied, int(order[rank]), last >= sorted_prefix(n0))


@dataclasses.dataclass(frozen=True)
class Picked:
    index: int         # the first index whose cdf exceeds the coin, n - 1 when none does
    fell: bool         # none did
    chunk: int         # the CHUNK the index is in


def categorical(probs, coin):
    """CategoricalSampler.java:33-44"""
    cdf = np.add.accumulate(np.asarray(probs, F32), dtype=F32)
    hit = np.flatnonzero(F32(coin) < cdf)
    index = int(hit[0]) if hit.size else cdf.size - 1
    return Picked(index, hit.size == 0, index // CHUNK)


def coin_for_rank(cs, cum, rank, edge="low"):
    """A coin whose product with `cum` selects `rank` of the cdf `cs` (cs[rank - 1] <= coin * cum < cs[rank]): the smallest such coin
    (edge low: the product is the first f32 not below cs[rank - 1], equal to it where the f32 grid allows, which is where the strict <
    decides) or the largest (edge high: the last product below cs[rank])."""
    cum = F32(cum)
    lo, hi = (F32(0.0) if rank == 0 else cs[rank - 1]), cs[rank]
    assert lo < hi
    if edge == "low":
        c = F32(lo / cum)
        while F32(c * cum) < lo:
            c = up(c)
        while c > 0 and F32(down(c) * cum) >= lo:
            c = down(c)
    else:
        c = min(F32(hi / cum), BELOW_ONE)
        while F32(c * cum) >= hi:
            c = down(c)
        while up(c) < 1 and F32(up(c) * cum) < hi:
            c = up(c)
    assert 0 <= c < 1 and lo <= F32(c * cum) < hi, (rank, edge, c)
    return F32(c)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    tag: str           # the boundary the case aims at
    logits: np.ndarray
    temperature: float
    topp: float        # outside (0, 1): categorical
    coin: float
    aim: dict          # what the oracle alone must show: keys of Sorted / Picked, plus subnormal, zero (counts among the probabilities)

    @property
    def V(self):
        return self.logits.size


# ------------------------------------------------------------------------------------------------ row builders
def two_level(V, K, step=STEP, block=0, pair=False):
    """(logits, idx): K distinct-valued logits 0, -step, -2 step, .. at shuffled indices idx (rank j of the descending order stands at
    idx[j]), everything else at LOW.  block > 0: ranks K - 3 - block .. K - 4 are equal instead (a tied block behind a distinct head, three
    distinct values behind it: the heap's own tail); pair: ranks 0 and 1 are equal."""
    rng = np.random.default_rng(100003 * V + 7 * K + block)
    idx = rng.permutation(V)[:K]
    lg = np.full(V, LOW, F32)
    vals = -(np.arange(K, dtype=F32) * F32(step))
    if block:
        vals[K - 3 - block:K - 3] = vals[K - 3 - block]
    if pair:
        vals[1] = vals[0]
    lg[idx] = vals
    return lg, idx


def distinct_candidates(lg, idx, temperature=1.0):
    """probabilities of a two_level row; asserts the K candidates are pairwise distinct as f32 probabilities and strictly descending in
    rank order, and that everything else is (far) below them"""
    p = probs_of(lg, temperature)
    sv = p[idx]
    assert np.all(sv[:-1] > sv[1:]), "candidates collide as f32 probabilities"
    rest = np.delete(p, idx)
    assert rest.size == 0 or rest.max() < sv[-1] * F32(1e-12)
    return p


def never_exceeds_row(V, K):
    """A two_level row whose K candidates' sequential f32 sum S, in descending order, is below 1: with topp = S the sum never EXCEEDS topp
    (> is strict) and every candidate is kept.  A sequential f32 sum loses or gains mass by rounding; the spacing of the candidates is varied
    until it loses some.  The cutoff depends on topp, so the candidate count is re-derived under topp = S until it is stable.
    Returns (logits, idx, S) or None when no spacing of the 24 tried gives S < 1 (K = 1: the one probability is 1.0)."""
    for s in range(24):
        lg, idx = two_level(V, K, step=F32(STEP * F32(1.0 + s / 16.0)))
        p = distinct_candidates(lg, idx)
        topp = F32(0.9)
        for _ in range(4):
            order, cs = sorted_candidates(p, topp)
            if cs[-1] == topp:
                break
            topp = cs[-1]
            if not 0 < topp < 1:
                break
        if 0 < topp < 1 and order.size == K and cs[-1] == topp:
            return lg, idx, F32(topp)
    return None


def generic_row(V, seed, scale=1.5):
    return (np.random.default_rng(seed).standard_normal(V) * scale).astype(F32)


def categorical_row(V):
    """A random row (sigma 1.5) whose sequential f32 total stays below 1 (the seed is searched), with probabilities that are exact zeros
    at the last indices (so the fall-through's V - 1 is not where the cdf stops growing) and raised logits on both sides of every chunk
    edge and in the last 16 elements (so the cdf moves by far more than an f32 step there)."""
    tail = 2 if V == 16 else 4
    for seed in range(64):
        lg = generic_row(V, 7000 + 97 * V + seed)
        lg[V - tail:] = F32(-200.0)
        for e in range(CHUNK, V, CHUNK):
            lg[e - 2:e + 2] += F32(3.0)
        if V > 32:
            lg[V - 12:V - tail] += F32(3.0)
        p = probs_of(lg, 1.0)
        if np.add.accumulate(p, dtype=F32)[-1] < 1 and np.all(p[V - tail:] == 0):
            return lg
    raise AssertionError("no categorical row with a total below 1")


def spread_row(V, maxima):
    """logits spread evenly over 80 .. 104 below the maximum 0 (shuffled), the maximum at every index of `maxima`: at temperature 1 the
    probabilities are the numerators (the sum is 1.0), f32-subnormal from 87.34 below the maximum and zero from 103.98"""
    rng = np.random.default_rng(31 * V + len(maxima))
    lg = np.empty(V, F32)
    rest = np.setdiff1d(np.arange(V), maxima)
    lg[rest] = -rng.permutation(np.linspace(80.0, 104.0, rest.size)).astype(F32)
    lg[list(maxima)] = F32(0.0)
    return lg


def subnormal_and_zero(logits, temperature):
    """How many probabilities are f32-subnormal and how many are zero, from the exponents in float64 alone — for rows whose softmax sum
    is exactly 1.0 (spread_row at temperature <= 1), where a probability is its numerator (float) exp(v - max)."""
    v = (np.asarray(logits, F32) / F32(temperature)).astype(F32)
    d = (v - v.max()).astype(np.float64)
    tiny, half_least = np.log(2.0) * -126, np.log(2.0) * -150          # below 2^-126: subnormal; below 2^-150: rounds to 0
    return int(np.count_nonzero((d < tiny) & (d > half_least))), int(np.count_nonzero(d < half_least))


def cutoff_row(V):
    """(logits, topp, index): a random row and a topp whose cutoff (1 - topp) / (V - 1) EQUALS the probability at `index` — a candidate
    by `>=`, the smallest one.  1 - topp is exact for topp in [0.5, 1) (a multiple of 2^-24); the quotient's grid is then about as fine as
    the probabilities' near (1 - topp) = 0.5, so the search runs over probabilities near 0.4 / (V - 1) and the few 1 - topp around each."""
    lg = generic_row(V, 9100 + V, scale=1.0)
    p = probs_of(lg, 1.0)
    near = np.flatnonzero((p > F32(0.3) / F32(V - 1)) & (p < F32(0.5) / F32(V - 1)))
    for j in near[np.argsort(-p[near], kind="stable")]:
        x0 = np.round(np.float64(F32(p[j] * F32(V - 1))) * 2.0 ** 24)
        for dx in range(-3, 4):
            topp = F32(1.0 - (x0 + dx) / 2.0 ** 24)
            if 0.5 <= topp < 1 and cutoff_of(topp, V) == p[j]:
                return lg, topp, int(j)
    raise AssertionError("no probability of the row is a cutoff")


# ------------------------------------------------------------------------------------------------ the case table
def _count_cases(V, K):
    """Two-level rows with exactly K candidates: n0 = K on both sides of the naive / exact split and of the chunk edge, the truncation
    rank placed by topp, the coin placed by the cdf."""
    out = []
    lg, idx = two_level(V, K)
    p = distinct_candidates(lg, idx)
    _, cs = sorted_candidates(p, 0.9)
    assert cs.size == K

    def add(tag, topp, coin, n0=K, **aim):
        aim = dict(tied=False, **aim, **({"n0": n0, "heap_tail": aim["last"] >= sorted_prefix(n0)} if n0 else {"heap_tail": False}))
        out.append(Case(f"{tag} V={V} K={K}", lg, 1.0, float(topp), float(coin), aim))

    first = int(np.flatnonzero(cs > F32(0.9))[0])
    add("count", 0.9, 0.5, last=first, exceeded=True)
    # truncation at rank 0, one f32 step under the top probability (so small a topp raises the cutoff: fewer than K candidates); the largest
    # coin: coin * cum is one f32 step under cum, the closest a draw comes to the fall-through (fl(coin * cum) < cum for every coin < 1)
    add("trunc-rank0", down(cs[0]), BELOW_ONE, n0=None, last=0, exceeded=True, rank=0, index=int(idx[0]))
    if K >= 2:
        # topp EQUAL to the cumulative sum at rank K - 2: not exceeded there (strict >), exceeded at the last rank
        add("trunc-last/coin-last", cs[K - 2], coin_for_rank(cs, cs[K - 1], K - 1), last=K - 1, exceeded=True, rank=K - 1, fell=False, index=int(idx[K - 1]))
        add("trunc-last/coin-first", cs[K - 2], 0.0, last=K - 1, exceeded=True, rank=0, fell=False, index=int(idx[0]))
        mid = K // 2
        add("trunc-last/coin-mid-high", cs[K - 2], coin_for_rank(cs, cs[K - 1], mid, "high"), last=K - 1, exceeded=True, rank=mid, index=int(idx[mid]))
    if K >= 5:
        # the last rank of the sorted prefix (the last truncation point the device answers) and the first of the heap's own tail
        add("trunc-prefix-last", cs[K - 5], coin_for_rank(cs, cs[K - 4], K - 4), last=K - 4, exceeded=True, rank=K - 4, fell=False, index=int(idx[K - 4]))
        add("trunc-prefix-last/coin-mid", cs[K - 5], coin_for_rank(cs, cs[K - 4], (K - 4) // 2, "high"), last=K - 4, exceeded=True, rank=(K - 4) // 2,
            index=int(idx[(K - 4) // 2]))
        add("trunc-tail-first", cs[K - 4], coin_for_rank(cs, cs[K - 3], K - 3), last=K - 3, exceeded=True, rank=K - 3)
    for edge in range(CHUNK, K, CHUNK):
        # the truncation rank as the last rank of a chunk and as the first of the next; phase 1 then ends at the chunk's end or one rank past it
        add("trunc-chunk-last", cs[edge - 2], coin_for_rank(cs, cs[edge - 1], edge - 1), last=edge - 1, exceeded=True, rank=edge - 1, index=int(idx[edge - 1]))
        add("trunc-chunk-first", cs[edge - 1], coin_for_rank(cs, cs[edge], edge), last=edge, exceeded=True, rank=edge, index=int(idx[edge]))
        # the truncation past the edge; the coin on either side of the chunk edge, as close to the cdf at the edge as f32 allows
        if K - 4 > edge:
            add("coin-chunk-last", cs[K - 5], coin_for_rank(cs, cs[K - 4], edge - 1, "high"), last=K - 4, exceeded=True, rank=edge - 1, index=int(idx[edge - 1]))
            add("coin-chunk-first", cs[K - 5], coin_for_rank(cs, cs[K - 4], edge), last=K - 4, exceeded=True, rank=edge, index=int(idx[edge]))
    return out


def _never_cases(V, K):
    got = never_exceeds_row(V, K)
    if got is None:
        return []
    lg, idx, S = got
    _, cs = sorted_candidates(probs_of(lg, 1.0), S)
    mk = lambda tag, topp, coin, **aim: Case(f"{tag} V={V} K={K}", lg, 1.0, float(topp), float(coin), dict(n0=K, tied=False, heap_tail=True, **aim))
    return [
        # coin * S for the largest coin is one f32 step under S: the last rank
        mk("never-exceeds/coin-top", S, BELOW_ONE, last=K - 1, exceeded=False, rank=K - 1, index=int(idx[K - 1])),
        mk("never-exceeds/coin-first", S, 0.0, last=K - 1, exceeded=False, rank=0, fell=False, index=int(idx[0])),
        mk("never-exceeds/coin-last", S, coin_for_rank(cs, S, K - 1), last=K - 1, exceeded=False, rank=K - 1, fell=False, index=int(idx[K - 1])),
        # the f32 just below S is exceeded exactly at the last rank
        mk("just-below-sum", down(S), coin_for_rank(cs, S, K // 2), last=K - 1, exceeded=True, rank=K // 2, fell=False, index=int(idx[K // 2])),
    ]


def _categorical_cases(V):
    lg = categorical_row(V)
    cdf = np.add.accumulate(probs_of(lg, 1.0), dtype=F32)
    tail = 2 if V == 16 else 4
    mk = lambda tag, coin, **aim: Case(f"cat/{tag} V={V}", lg, 1.0, 0.0, float(coin), aim)
    out = [mk("coin-zero", 0.0, index=0, fell=False, chunk=0),
           mk("coin-mid", 0.5, fell=False),
           # the row's total is below 1 and the last `tail` probabilities are 0: no cdf exceeds the largest coin
           mk("fall-through", BELOW_ONE, index=V - 1, fell=True),
           # the last index the cdf still grows at
           mk("last-positive", down(cdf[-1]), index=V - tail - 1, fell=False)]
    for e in range(CHUNK, V, CHUNK):
        c = e // CHUNK
        out += [mk(f"chunk{c - 1}-end", cdf[e - 1], index=e, fell=False, chunk=c),          # strict <: equal to the cdf at the end of the chunk
                mk(f"chunk{c - 1}-end-below", down(cdf[e - 1]), index=e - 1, fell=False, chunk=c - 1),
                mk(f"chunk{c - 1}-end-above", up(cdf[e - 1]), index=e, fell=False, chunk=c)]
    if V > 32:
        out.append(mk("last-16", cdf[V - 10], index=V - 9, fell=False, chunk=(V - 9) // CHUNK))      # V = 4112: inside the 16-element chunk
    return out


def _tie_cases(V):
    shapes = [(5, 4)] if V == 16 else [(600, 300)] + ([(CHUNK - 1, 5)] if V > CHUNK + 4 else [])
    out = []
    for H, B in shapes:
        K = H + B + 3                                   # a distinct head, the tied block, three distinct values (the heap's own tail)
        lg, idx = two_level(V, K, block=B)
        p = probs_of(lg, 1.0)
        _, cs = sorted_candidates(p, 0.9)
        assert cs.size == K
        topp, cum = cs[K - 5], cs[K - 4]                # exceeded at the block's last rank, the last of the sorted prefix: every rank up to it can be drawn
        mk = lambda tag, rank, **aim: Case(f"tie/{tag} V={V} H={H} B={B}", lg, 1.0, float(topp), float(coin_for_rank(cs, cum, rank)),
                                           dict(n0=K, last=K - 4, exceeded=True, heap_tail=False, rank=rank, **aim))
        out += [mk("head", H // 2, tied=False, index=int(idx[H // 2])),               # ties elsewhere in the row: the device answers
                mk("head-last", H - 1, tied=False, index=int(idx[H - 1])),             # borders the tied block, is itself not tied
                mk("block-first", H, tied=True),                                       # only rank r + 1 equals it
                mk("block-last", K - 4, tied=True)]                                    # only rank r - 1 equals it; the last rank the cdf walk sees
        lg2, idx2 = two_level(V, K, block=B, pair=True)
        _, cs2 = sorted_candidates(probs_of(lg2, 1.0), 0.9)
        out += [Case(f"tie/top-pair V={V} H={H} B={B}", lg2, 1.0, float(cs2[K - 5]), 0.0, dict(n0=K, rank=0, tied=True, heap_tail=False)),      # r = 0: only r + 1
                Case(f"tie/behind-top-pair V={V} H={H} B={B}", lg2, 1.0, float(cs2[K - 5]), float(coin_for_rank(cs2, cs2[K - 4], 2)),
                     dict(n0=K, rank=2, tied=False, heap_tail=False, index=int(idx2[2])))]
    if V > 16:
        lg, topp, j = cutoff_row(V)
        p = probs_of(lg, 1.0)
        out.append(Case(f"cutoff-equal V={V}", lg, 1.0, float(topp), 0.5,
                        dict(n0=int(np.count_nonzero(p > p[j])) + 1, tied=False, heap_tail=False, cutoff_index=j)))
    return out


def _value_cases(V):
    last_chunk = ((V - 1) // CHUNK) * CHUNK
    places = {"max-first": (0,), "max-last": (V - 1,), "max-triple": (3, V // 2, V - 2)}
    if last_chunk:
        places["max-last-chunk"] = (last_chunk,)
    out = []
    for name, maxima in places.items():
        lg = spread_row(V, maxima)
        single = len(maxima) == 1
        if not single:
            lg[maxima[1]] = F32(-0.0)            # a negative zero among positive-zero maxima: equal to them, exp(-0 - 0) = 1
        for T in (1.0, 0.02, 5.0):
            aim = {}
            if T <= 1.0 and single:              # the softmax sum is 1.0: a probability is its numerator
                sub, zero = subnormal_and_zero(lg, T)
                aim = dict(subnormal=sub, zero=zero)
            tag = f"value/{name} T={T} V={V}"
            # coin 0: the first index with a positive probability, a subnormal one at T = 1 unless the maximum stands at index 0
            out.append(Case(tag + " cat0", lg, T, 0.0, 0.0, dict(aim, fell=False)))
            out.append(Case(tag + " cat-top", lg, T, 1.0, float(BELOW_ONE), dict(aim)))
            topp_aim = dict(aim, tied=not single)
            if T <= 1.0:
                topp_aim.update(n0=len(maxima), rank=0 if single else None)      # everything else is 80 / T below the maximum
                if single:
                    topp_aim.update(index=int(maxima[0]), last=0, exceeded=True, heap_tail=False)
            out.append(Case(tag + " topp", lg, T, 0.9, 0.5, {k: v for k, v in topp_aim.items() if v is not None}))
    # a maximum of +0 over negative logits down to -0: the sign of zero does not reach the probabilities
    lg = -np.abs(generic_row(V, 4400 + V))
    lg[V // 2], lg[1] = F32(0.0), F32(-0.0)
    out.append(Case(f"value/zero-maximum V={V}", lg, 0.7, 0.95, 0.25, {}))
    # very small and large temperatures on an ordinary row
    lg = generic_row(V, 4500 + V, scale=3.0)
    for T, topp, coin in ((0.02, 0.95, 0.37), (0.02, 0.0, 0.61), (5.0, 0.95, 0.37), (5.0, 0.0, 0.999)):
        out.append(Case(f"value/temperature T={T} topp={topp} V={V}", lg, T, topp, coin, {}))
    return out


def stability_cases(V):
    """Every candidate equal except one larger value at a middle index: the sort must carry it to rank 0 through four stable passes over
    V - 1 equal keys; coins on rank 0 (its lowest and its highest) are answered on the device, with that index and no tie flag."""
    lg = np.zeros(V, F32)
    j = (V // 2 + 1) % V
    lg[j] = F32(1.0)
    p = probs_of(lg, 1.0)
    _, cs = sorted_candidates(p, 0.5)                # topp 0.5: the truncation is in the sorted prefix at every V
    s = sorted_topp(p, 0.5, 0.0)
    aim = dict(n0=V, rank=0, tied=False, heap_tail=False, index=j)
    return [Case(f"stability/coin-zero V={V}", lg, 1.0, 0.5, 0.0, aim),
            Case(f"stability/coin-rank0-top V={V}", lg, 1.0, 0.5, float(coin_for_rank(cs, s.cum, 0, "high")), aim),
            Case(f"stability/coin-rank1 V={V}", lg, 1.0, 0.5, float(coin_for_rank(cs, s.cum, 1)), dict(n0=V, rank=1, tied=True, heap_tail=False))]


@functools.lru_cache(maxsize=None)
def cases(V):
    """The table for one vocabulary.  Rows are shared between the cases built on them and must not be written to."""
    out = []
    for K in COUNTS + EXTRA_COUNTS.get(V, ()):
        if K < V:
            out += _count_cases(V, K)
            out += _never_cases(V, K)
    out += _categorical_cases(V) + _tie_cases(V) + _value_cases(V) + stability_cases(V)
    for c in out:
        c.logits.setflags(write=False)
        assert np.all(np.isfinite(c.logits))
    return tuple(out)
