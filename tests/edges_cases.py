"""Signals, options and the comparison shared by tests/test_edges_host.py and
tests/test_gpu_edges.py (the edges pass, csrc/edges.h)."""
import numpy as np

from msgpu.edges import TILE as T
from msgpu.edges import Edges, edges_reference, gains, loop_gains, threshold

SR = 48000
TRIM_DB = -60.0
THR = threshold(TRIM_DB)
N = 3 * T + 5
LENGTHS = (0, 1, 2, T - 1, T, T + 1, N)
FLOOR = 1e-4          # the level of what counts as silence at TRIM_DB

# every option the pass has, each at least once; 2 / 20 ms are 96 / 960 frames, 300 ms more than any signal here
CONFIGS = {
    "both": Edges(trim_db=TRIM_DB, pad_ms=1, fade_ms=(2, 20)),
    "head linear": Edges(trim_db=TRIM_DB, sides="head", pad_ms=1, fade_ms=(2, 20), curve="linear"),
    "tail qsin": Edges(trim_db=TRIM_DB, sides="tail", pad_ms=1, fade_ms=(2, 20), curve="qsin"),
    "pads clip": Edges(trim_db=TRIM_DB, pad_ms=(5, 5)),
    "fades clip": Edges(trim_db=TRIM_DB, fade_ms=(2, 20)),              # a single sound frame: len = 1
    "fades only": Edges(fade_ms=(2, 20), curve="qsin"),
    "fades longer than the signal": Edges(fade_ms=(300, 100)),
    "fade-in only": Edges(trim_db=TRIM_DB, fade_ms=(300, 0), curve="linear"),
    "loop": Edges(trim_db=TRIM_DB, loop_ms=50),
    "loop longer than half": Edges(trim_db=TRIM_DB, pad_ms=(0, 1), loop_ms=1000, curve="linear"),
    "loop only": Edges(loop_ms=10, curve="qsin"),
    "threshold underflows": Edges(trim_db=-2000.0, fade_ms=1),
    "threshold one": Edges(trim_db=0.0, sides="tail"),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def wave_edge(channels):
    """The last frame of the find kernel's lane 63 and the first of lane 64 in a tile whose first
    float is 16-byte aligned: a lane reads one piece of four floats."""
    f = 64 * 4 // channels
    return f - 1, f


def signals(channels):
    """[(name, x)]: x float32 (n,) or (n, 2)."""
    rng = np.random.default_rng(20240607 + channels)
    shape = (lambda n: (n,)) if channels == 1 else (lambda n: (n, 2))

    def floor(n):
        return (rng.uniform(-FLOOR, FLOOR, shape(n))).astype(np.float32)

    def loud(n):
        v = rng.uniform(0.01, 1.0, shape(n)) * rng.choice([-1.0, 1.0], shape(n))
        return v.astype(np.float32)

    out = []
    for n in LENGTHS:
        x = floor(n)
        if n >= 4:
            x[n // 4:n // 2] = loud(n // 2 - n // 4)
        elif n:
            x[0] = 0.5
        out.append((f"burst n={n}", x))
    for f in (0, N - 1, T - 1, T):
        x = floor(N)
        x[f] = -0.25
        out.append((f"one sound frame at {f}", x))
    below = np.nextafter(THR, np.float32(0))
    assert below < THR and below.dtype == np.float32
    for name, v in (("at the threshold", THR), ("one ulp below the threshold", below)):
        x = np.zeros(shape(N), dtype=np.float32)
        x[100] = -v
        out.append((name, x))
    a, b = wave_edge(channels)
    for name, fr in (("last lane of a wave", (a,)), ("first lane of the next wave", (b,)), ("both sides of a wave", (a, b))):
        x = np.zeros(shape(T + 8), dtype=np.float32)      # a multiple of four frames: packed with a gap of four, every one is aligned
        for f in fr:
            x[f] = THR
        out.append((name, x))
    x = np.zeros(shape(N), dtype=np.float32)
    x[10:20] = np.nan
    x[500] = np.inf
    x[900] = -np.inf
    x[N - 30:] = np.nan
    out.append(("NaN and inf frames", x))
    out.append(("all silent", floor(N)))
    out.append(("all zero", np.zeros(shape(T + 1), dtype=np.float32)))
    x = floor(N)
    x[3] = 0.5
    x[N - 2] = 0.5
    out.append(("pads clip at both ends", x))
    x = floor(2 * T + 1)                                  # an odd span from a trim without pads
    x[T - 100:T + 901] = loud(1001)
    out.append(("odd span", x))
    if channels == 2:
        x = floor(N)
        x[1000:2000, 1] = loud(1000)[:, 1]
        out.append(("sound in R only", x))
        x = floor(T)
        x[300:310, 0] = np.nan
        x[300:310, 1] = 0.5
        out.append(("NaN in L, sound in R", x))
    return out


def library_reference(x, e):
    """edges_reference with the library's own float32 gains: the definition's arithmetic around them."""
    return edges_reference(x, SR, e, gains=gains, loop_gains=loop_gains)


def assert_same(what, y, rec, y_want, rec_want):
    assert rec.tobytes() == rec_want.tobytes(), f"{what}: record {rec} != {rec_want}"
    assert y.shape == y_want.shape and y.dtype == np.float32
    bad = np.flatnonzero(bits(y).ravel() != bits(y_want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:4]}"
