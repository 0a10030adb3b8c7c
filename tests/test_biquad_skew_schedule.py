"""The slot schedule of biquad_pipe_skew1 (asdr_kernels.hip: the 4-stage DF1 cascade on four lanes with ONE sample of stage skew, the form of
the plain kind's audio cascades) as a lock-step emulation in numpy float32, against the plain stage-major cascade, bit for bit.

The emulation follows the kernel step by step: at slot t = 0..130 lane `st` handles sample t - st; stage 0 takes its sample from the
chunk of the row it read one step ahead, stage k > 0 takes what its left neighbour's y1 register held at the END of the previous slot;
state updates are predicated in the fill (0..2) and drain (128..130) slots only; stage 3 keeps its outputs in registers and writes chunk
c - 1 of the SAME row behind step c (five samples carried over from step c - 1, three from step c), the last chunk behind the drain.
An index, hand-off or in-place ordering mistake in that schedule shows here, without a GPU.  Two consecutive blocks, so that the carried
x1, x2, y1, y2 of every stage cross a block boundary."""
import numpy as np
import pytest

N, NST = 128, 4
f32 = np.float32


def _coefficients(rng, rows):
    """(rows, 4 stages, 5): b0, b1, b2, a1, a2 (CMSIS sign convention: the a's are ADDED) of stable sections, poles at radius 0.5..0.97"""
    r = rng.uniform(0.5, 0.97, (rows, NST)); th = rng.uniform(0.1, 3.0, (rows, NST))
    cf = np.empty((rows, NST, 5), f32)
    cf[..., 0:3] = rng.uniform(-1.0, 1.0, (rows, NST, 3))
    cf[..., 3] = 2.0 * r * np.cos(th); cf[..., 4] = -r * r
    return cf


def _reference(x, cf, sv):
    """arm_biquad_cascade_df1_f32: stage-major over the block, acc = b0 x; += b1 x1; += b2 x2; += a1 y1; += a2 y2, every operation rounded.
    x (rows, 128), cf (rows, 4, 5), sv (rows, 4, 4) = x1, x2, y1, y2 per stage, updated in place.  Returns the filtered rows."""
    cur = x.copy()
    for st in range(NST):
        b0, b1, b2, a1, a2 = (cf[:, st, k] for k in range(5))
        x1, x2, y1, y2 = (sv[:, st, k].copy() for k in range(4))
        out = np.empty_like(cur)
        for n in range(N):
            xi = cur[:, n]
            acc = b0 * xi; acc = acc + b1 * x1; acc = acc + b2 * x2; acc = acc + a1 * y1; acc = acc + a2 * y2
            x2, x1, y2, y1 = x1, xi, y1, acc
            out[:, n] = acc
        sv[:, st, 0], sv[:, st, 1], sv[:, st, 2], sv[:, st, 3] = x1, x2, y1, y2
        cur = out
    return cur


def _skew1(row, cf, sv, carry=3):
    """biquad_pipe_skew1 on lanes 0..3 (lane = stage), all rows at once: row (rows, 128) is filtered IN PLACE, sv updated in place.
    carry = 3: stage 3 runs three samples behind the slots (any other value is a wrong schedule, for the test of the test)."""
    b0, b1, b2, a1, a2 = (cf[:, :, k].copy() for k in range(5))            # per lane
    x1, x2, y1, y2 = (sv[:, :, k].copy() for k in range(4))
    stage = np.arange(NST)[None, :]

    def slot(t, xin, edge):
        nonlocal x1, x2, y1, y2
        d = np.zeros_like(y1); d[:, 1:] = y1[:, :-1]                       # row_shr:1 of the neighbours' y1 as the previous slot left it
        x = np.where(stage == 0, xin[:, None], d)
        acc = b0 * x; acc = acc + b1 * x1; acc = acc + b2 * x2; acc = acc + a1 * y1; acc = acc + a2 * y2
        n = t - stage
        act = ((n >= 0) & (n < N)) if edge else np.ones_like(n, bool)
        x2 = np.where(act, x1, x2); x1 = np.where(act, x, x1); y2 = np.where(act, y1, y2); y1 = np.where(act, acc, y1)
        return acc[:, 3].copy()                                            # (what stage 3 keeps for its write)

    with np.errstate(all="ignore"):                                        # (idle stages compute on whatever their registers hold)
        xn = row[:, 0:8].copy()
        nx = row[:, 8:16].copy()
        yp = [slot(j, xn[:, j], j < 3) for j in range(8)]                  # step 0: slots 0..2 fill
        xn = nx
        for c in range(1, 16):
            if c < 15:
                nx = row[:, 8 * (c + 1):8 * (c + 2)].copy()                # the next chunk, read before this step's write
            y = [slot(8 * c + j, xn[:, j], False) for j in range(8)]
            row[:, 8 * (c - 1):8 * c] = np.stack(yp[carry:8] + y[0:carry], axis=1)
            yp = y
            xn = nx
        y = [slot(N + j, np.zeros(len(row), f32), True) for j in range(3)]  # slots 128..130 drain
        row[:, N - 8:N] = np.stack((yp[carry:8] + y[0:carry] + [y[2]])[:8], axis=1)
    sv[:, :, 0], sv[:, :, 1], sv[:, :, 2], sv[:, :, 3] = x1, x2, y1, y2


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _inputs(kind, rng, rows):
    if kind == "random":
        return rng.uniform(-1.0, 1.0, (rows, 2, N)).astype(f32)
    if kind == "denormals":                                                # denormal samples, alone and between normal ones
        x = (rng.integers(-(1 << 22), 1 << 22, (rows, 2, N)).astype(np.int64) & 0x807FFFFF).astype(np.uint32).view(f32)
        x[::2, :, ::5] = rng.uniform(-1e-30, 1e-30, x[::2, :, ::5].shape).astype(f32)
        return x
    x = np.zeros((rows, 2, N), f32)                                        # the edge slots: only samples 0, 1, 2 and 125, 126, 127
    pos = [0, 1, 2, 125, 126, 127]
    for r in range(rows):
        for p in ([pos[r % 6]] if r < 6 else pos):
            x[r, :, p] = rng.uniform(-1.0, 1.0, 2).astype(f32)
    return x


@pytest.mark.parametrize("kind", ["random", "denormals", "edges"])
def test_one_sample_skew_equals_the_stage_major_cascade(kind):
    rng = np.random.default_rng({"random": 11, "denormals": 12, "edges": 13}[kind])
    rows = 24
    x = _inputs(kind, rng, rows)
    cf = _coefficients(rng, rows)
    sv0 = (rng.uniform(-1.0, 1.0, (rows, NST, 4)) * (1e-38 if kind == "denormals" else 1.0)).astype(f32)
    sv_ref, sv_got = sv0.copy(), sv0.copy()
    for blk in range(2):                                                   # the state of block 0 is what block 1 starts from
        want = _reference(x[:, blk], cf, sv_ref)
        row = x[:, blk].copy()
        _skew1(row, cf, sv_got)
        assert np.array_equal(_bits(row), _bits(want)), "block %d: samples %s" % (blk, np.argwhere(_bits(row) != _bits(want))[:4].tolist())
        assert np.array_equal(_bits(sv_got), _bits(sv_ref)), "block %d: carried state" % blk
    if kind == "denormals":
        assert ((np.abs(x) > 0) & (np.abs(x) < np.finfo(f32).tiny)).any()


def test_the_emulation_notices_a_wrong_schedule():
    """the same emulation with stage 3's write-back one sample off differs from the cascade: the comparison above can fail"""
    rng = np.random.default_rng(5)
    x = _inputs("random", rng, 4)[:, 0]
    cf = _coefficients(rng, 4)
    sv = np.zeros((4, NST, 4), f32)
    want = _reference(x, cf, sv.copy())
    for carry, same in ((3, True), (4, False), (2, False)):
        row = x.copy()
        _skew1(row, cf, sv.copy(), carry=carry)
        assert np.array_equal(_bits(row), _bits(want)) == same, carry
