"""The slot form of the pair kernel as resident waves that pull items (csrc/k1_queue.h; kernels.hip, k1w_pairs_slots) with the constant
emit for separated items (emit_constant): the launch has one workgroup per wave slot of the device, each takes items of the list from
eight counters until none is left, and an item whose tile and chunk are separated writes its words without counting or classifying row
by row.  The class table that leaves launch_k1 stays the identity order's and the oracle's bit for bit -- with more items than wave
slots, with one worker that steals everything, with a worker count that is no multiple of eight, with the one-item-per-workgroup launch
(REO_K1_QUEUE=0), with separated items at the padded edges, and on a context that builds again and again (the counters are cleared)."""
import numpy as np
import pytest

from slot_cases import masks as _masks   # the rule in numpy with the places kept: side = group id for comparison 0
from test_gpu_parity import _expected_block_codes, _setup
from test_gpu_slot_order import _identity_codes, _model

pytestmark = pytest.mark.gpu

WAVE_SLOTS = 256 * 4 * 3   # MI355X: 256 CUs x 4 SIMDs x 3 waves of the pair kernel


def _queue_env(monkeypatch, workers=None, queue=None):
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    for name, v in (("REO_K1_WORKERS", workers), ("REO_K1_QUEUE", queue)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _oracle_table(oracle, X, gid, ng, thr, seed):
    return oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, ng, 0, thr[:, 0].tolist(), seed)


_shared = {}


def _many_items(pkg, oracle, monkeypatch):
    """T0 8 193 x 64 once for the three cases below: the matrix, the model's counts, the identity order's table, the oracle's blocks"""
    if "many" not in _shared:
        G, S, seed = 8193, 64, 7
        X = pkg.synth.t0_ranks(G, S, seed)
        group = pkg.synth.groups(S)
        gid = pkg.encode_groups(group)[0]
        live, sep = _model(X, gid)
        blocks = [(0, 48, 0, 256), (0, 32, G - 256, G), (G - 40, G, 0, 128), (G - 64, G, G - 64, G), (4000, 4040, 4000, 4200), (8160, 8193, 8100, 8193)]
        _queue_env(monkeypatch)
        ctx, gid, ng = _setup(pkg, X, group, seed)
        with ctx:
            thr = ctx.get_thresholds()
        Xf = np.asfortranarray(X.astype(np.float64))
        expected = [_expected_block_codes(oracle, Xf, gid, thr, seed, *b) for b in blocks]
        identity = _identity_codes(pkg, X, group, seed, monkeypatch)
        _shared["many"] = (X, group, seed, live, sum(sum(v) for v in sep.values()), blocks, expected, identity)
    return _shared["many"]


@pytest.mark.parametrize("workers,queue", [(None, None), (8, None), (None, 0)])
def test_more_items_than_wave_slots(pkg, oracle, monkeypatch, workers, queue):
    """257 tiles x 33 chunks x 2 sides: more than twice as many list entries as the device has wave slots, so every worker of the default
    launch takes several items; eight workers take about a thousand each; REO_K1_QUEUE=0 is the one-item-per-workgroup launch."""
    X, group, seed, n_items, separated, blocks, expected, identity = _many_items(pkg, oracle, monkeypatch)
    G = X.shape[0]
    print("list entries by the model", n_items, "separated", separated)
    assert n_items > 2 * WAVE_SLOTS, "the shape has become too small for this test"
    assert n_items % WAVE_SLOTS > WAVE_SLOTS // 2, "no half-height items here: entries = live (tile, chunk, side) triples"
    assert separated > 0
    _queue_env(monkeypatch, workers, queue)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    with ctx:
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] == 2 * separated
        got = ctx.get_codes(0, G, 0, G)
    assert np.array_equal(got, identity), "class table differs from the identity order's"
    for (i0, i1, j0, j1), e in zip(blocks, expected):
        assert np.array_equal(got[i0:i1, j0:j1], e), (i0, i1, j0, j1)


@pytest.mark.parametrize("G,S", [(1000, 64), (2049, 66)])
@pytest.mark.parametrize("workers", [1, 13])
def test_few_workers_steal_everything(pkg, oracle, monkeypatch, G, S, workers):
    """One worker empties its own queue and then the seven others; thirteen (no multiple of eight) leave three labels with one worker
    and five with two.  1 000 x 64: half-height items in the list; 2 049 x 66: padded sample slots, padded genes, a one-gene last tile."""
    seed = 7
    X = pkg.synth.t0_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    _queue_env(monkeypatch, workers)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    with ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        assert ctx.info()["k1_slot_order"] == 1 and ctx.info()["k1_half_tiles_separated"] > 0
        got = ctx.get_codes(0, G, 0, G)
    assert np.array_equal(got, _oracle_table(oracle, X, gid, ng, thr, seed)), "class table differs from the oracle's"


def _planted_odd(seed=11):
    """test_gpu_slot_order._planted with a gene count that is no multiple of 32: 1 013 genes in classes of 254 / 253 / 253 / 253 on levels
    far apart, other bands per side.  The last chunk then ends in padding columns and the last tile in rows beyond G."""
    rng = np.random.default_rng(seed)
    G, S = 1013, 64
    # class -> band on side 0 / side 1, the sums (2, 3, 4, 5) in slot order.  Not _planted's bands: with runs of 254 / 253 slots a chunk
    # of 256 holds its class and the first genes of the next one, and those bands leave side 1 without a chunk below a tile.
    a = np.array([0, 2, 4, 1]); b = np.array([2, 1, 0, 4])
    cls = rng.permutation(np.repeat(np.arange(4), [254, 253, 253, 253]))
    sub = rng.integers(0, 2, size=G)
    X = np.empty((G, S), dtype=np.int64)
    for s in range(S):
        level = 2 * a[cls] + sub if s < S // 2 else 2 * b[cls] + 1 - sub
        X[:, s] = level * 1_000_000 + rng.permutation(G)
    return X


@pytest.mark.parametrize("queue", [None, 0])
def test_constants_at_the_edges(pkg, oracle, monkeypatch, queue):
    X = _planted_odd()
    G, S = X.shape
    seed = 3
    group = pkg.synth.groups(S)
    gid = pkg.encode_groups(group)[0]
    is_live, sep = _masks(X, gid)
    NT, NQ = is_live.shape
    assert G % 32 != 0 and 32 * NT > G and 256 * NQ > G
    assert all(m.any() for side in (0, 1) for m in sep[side]), "both constants on both sides"
    anysep = sep[0][0] | sep[0][1] | sep[1][0] | sep[1][1]
    assert anysep[:, NQ - 1].any(), "a separated item in the last chunk (padding columns)"
    # The last tile (rows beyond G) lies inside the last chunk, its own, and live items have no chunk left of the tile's: by the rule
    # (k1_slots.h: a tile inside its chunk never qualifies) an item with rows beyond G is never separated, for any gene count.  Its
    # rows are emitted by emit_gene next to the constant words of the last chunk's columns, which the whole-table comparison covers.
    assert (NT - 1) // 8 == NQ - 1 and not anysep[NT - 1, :].any()
    # every item of a list that fills at most half of the wave slots is dealt as two half-height items (k1_items.h)
    assert 0 < 2 * int(is_live.sum()) <= WAVE_SLOTS // 2, "a separated item is half-height"
    total = sum(int(m.sum()) for side in (0, 1) for m in sep[side])
    _queue_env(monkeypatch, None, queue)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    with ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] == 2 * total
        got = ctx.get_codes(0, G, 0, G)
    assert np.array_equal(got, _oracle_table(oracle, X, gid, ng, thr, seed)), "class table differs from the oracle's"


def test_counters_are_reset_between_builds(pkg, oracle, monkeypatch):
    """One context, three builds: A, then B through set_matrix, then A again.  A launch leaves every counter beyond its queue's length;
    a counter that was not cleared hands out no item, and the table stays as the clear in front of the launch left it."""
    G, S = 2049, 66
    group = pkg.synth.groups(S)
    XA, XB = pkg.synth.t0_ranks(G, S, 7), pkg.synth.t0_ranks(G, S, 8)
    assert not np.array_equal(XA, XB)
    _queue_env(monkeypatch)
    ctx, gid, ng = _setup(pkg, XA, group, 7)
    expected = {}
    with ctx:
        for name, X in (("A", XA), ("B", XB), ("A", XA)):
            if expected:
                ctx.set_matrix(X)
                ctx.set_groups(gid, ng)
                ctx.compute_thresholds(0.01)
            thr = ctx.get_thresholds()
            ctx.build_pairs(0)
            assert ctx.info()["k1_slot_order"] == 1
            if name not in expected:
                expected[name] = _oracle_table(oracle, X, gid, ng, thr, 7)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), expected[name]), "build of matrix " + name
    assert not np.array_equal(expected["A"], expected["B"])


def test_end_to_end_equal_with_and_without_queue(pkg, monkeypatch):
    """identify_degs at 2 049 x 66, 16 forced passes: result, trace and iteration count identical under REO_K1_QUEUE=1 and 0."""
    G, S, seed = 2049, 66, 7
    X = pkg.synth.t0_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 300, seed)
    out = {}
    for queue in ("1", "0"):
        _queue_env(monkeypatch, None, queue)
        ctx, gid, ng = _setup(pkg, X, group, seed)
        with ctx:
            ctx.build_pairs(0)
            assert ctx.info()["k1_slot_order"] == 1
            out[queue] = ctx.identify_degs(ref0, 1.0, 0.05, 16, 0)
    (r1, i1, t1), (r0, i0, t0) = out["1"], out["0"]
    assert i1 == i0 == 16
    assert np.array_equal(np.asarray(t1), np.asarray(t0), equal_nan=True)
    assert np.array_equal(r1, r0, equal_nan=True)
