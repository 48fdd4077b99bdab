"""Slot order of the pair kernel (csrc/k1_slots.h; kernels.hip, launch_k1): tie-free data of two groups on one shard is counted with the
genes ordered by level, items whose i-tile and wave chunk are separated on their side skip the count loop, and the class table that
leaves launch_k1 is the identity order's bit for bit.  Every case compares the table with the oracle's and / or with a context created
under REO_K1_SLOTS=0; the number of separated items is modelled here in numpy from the rule alone and compared with
info()["k1_half_tiles_separated"] (a full item counts 2, a half-height item 1)."""
import numpy as np
import pytest

from slot_cases import model as _model, model_count as _model_count   # the rule in numpy: side = group id for comparison 0
from test_gpu_parity import _eager_ctx, _expected_block_codes, _setup

pytestmark = pytest.mark.gpu


def _identity_codes(pkg, X, group, seed, monkeypatch, blocks=None):
    """the table (or blocks of it) of a context created with REO_K1_SLOTS=0"""
    monkeypatch.setenv("REO_K1_SLOTS", "0")
    try:
        ctx, gid, ng = _setup(pkg, X, group, seed)
        with ctx:
            ctx.build_pairs(0)
            assert ctx.info()["k1_slot_order"] == 0 and ctx.info()["k1_half_tiles_separated"] == 0
            G = X.shape[0]
            return ctx.get_codes(0, G, 0, G) if blocks is None else [ctx.get_codes(*b) for b in blocks]
    finally:
        monkeypatch.delenv("REO_K1_SLOTS")


@pytest.mark.parametrize("G,S,by_issue", [(1000, 64, 152), (2049, 66, 970)])
def test_t0_table_counts_and_separated_items(pkg, oracle, monkeypatch, G, S, by_issue):
    """T0 1 000 x 64 (12 planes; every item in the last round: half-height items) and 2 049 x 66 (15 planes, 33 samples per side: padding
    sample slots, padded genes, a one-gene last tile)."""
    seed = 7
    X = pkg.synth.t0_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    Xf = np.asfortranarray(X.astype(np.float64))
    model = _model_count(X, gid)
    print("separated items by the model", model, "-> half tiles", 2 * model)
    assert model > 0 and 2 * model == by_issue
    with ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        print("k1_slot_order", info["k1_slot_order"], "k1_half_tiles_separated", info["k1_half_tiles_separated"])
        assert info["k1_slot_order"] == 1 and info["has_ties"] == 0
        assert info["k1_half_tiles_separated"] == 2 * model
        got = ctx.get_codes(0, G, 0, G)
        assert np.array_equal(got, oracle.build_codes(Xf, gid, ng, 0, thr[:, 0].tolist(), seed)), "class table differs from the oracle"
        for blk in [(0, 40, G - 300, G), (G - 33, G, 0, 64)]:   # the planes stay in gene order
            gt, eq = ctx.pair_counts(*blk)
            egt, eeq = oracle.pair_counts(Xf, gid, ng, *blk)
            assert np.array_equal(gt, egt) and np.array_equal(eq, eeq)
    assert np.array_equal(got, _identity_codes(pkg, X, group, seed, monkeypatch)), "class table differs from the identity order's"


def _planted(seed=11):
    """1 024 genes x 64 samples on 8 levels far apart per side, file order shuffled.  The levels of the two sides are different
    permutations of the genes' classes, so that chunks later in slot order lie BELOW earlier tiles on one side: both constants occur."""
    rng = np.random.default_rng(seed)
    G, S = 1024, 64
    a = np.array([1, 0, 3, 2]); b = np.array([0, 2, 1, 3])   # class -> band on side 0 / side 1 (sums 1, 2, 4, 5: four runs of 256 slots)
    cls = rng.permutation(np.repeat(np.arange(4), 256))
    sub = rng.integers(0, 2, size=G)
    X = np.empty((G, S), dtype=np.int64)
    for s in range(S):
        level = 2 * a[cls] + sub if s < S // 2 else 2 * b[cls] + 1 - sub   # (the half level changes sides: it cancels in the key)
        X[:, s] = level * 1_000_000 + rng.permutation(G)
    return X


def test_planted_levels(pkg, oracle, monkeypatch):
    X = _planted()
    G, S = X.shape
    seed = 3
    group = pkg.synth.groups(S)
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    live, sep = _model(X, gid)
    print("live items", live, "separated items by side [n_side, 0]", sep)
    total = sum(sum(v) for v in sep.values())
    assert total > live // 2, "most tiles separated"
    assert all(v > 0 for side in (0, 1) for v in sep[side]), "both constants on both sides"
    with ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] == 2 * total
        code = oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, ng, 0, thr[:, 0].tolist(), seed)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), code)


def test_nothing_separable(pkg, oracle, monkeypatch):
    """Every column is the same permutation of the genes plus noise: the permutation's levels are confined to a band as narrow as the
    noise is wide, so every gene's positions range over most of a sample and no tile lies apart from any chunk."""
    G, S, seed = 1000, 64, 5
    rng = np.random.default_rng(seed)
    base = rng.permutation(G)
    X = (base[:, None] + rng.integers(0, 64 * G, size=(G, S))) * G + np.arange(G)[:, None]   # (the gene breaks every tie)
    group = pkg.synth.groups(S)
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    assert _model_count(X, gid) == 0
    with ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] == 0 and info["has_ties"] == 0
        code = oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, ng, 0, thr[:, 0].tolist(), seed)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), code)


@pytest.mark.parametrize("case", ["ties", "three_groups", "shard", "pipelined_upload"])
def test_fallbacks_keep_the_identity_order(pkg, oracle, monkeypatch, case):
    """What the slot order does not cover runs the identity order: k1_slot_order stays 0 and the table is the oracle's."""
    G, S, seed = (2049, 66, 9) if case == "shard" else (1000, 64, 9)   # (three work units: shard 0 of 2 owns two of them)
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    X = pkg.synth.t1_counts(G, S, seed) if case == "ties" else pkg.synth.t0_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    if case == "three_groups":
        group = np.array(["a"] * 20 + ["b"] * 22 + ["c"] * 22, dtype=object)
    Xf = np.asfortranarray(X.astype(np.float64))
    if case == "pipelined_upload":
        monkeypatch.setenv("REO_EAGER_UPLOAD", "2")
        ctx = _eager_ctx(pkg, np.asfortranarray(X), group, seed)
        gid, ng = pkg.encode_groups(group)[0], 2
    else:
        ctx, gid, ng = _setup(pkg, X, group, seed)
    with ctx:
        thr = ctx.get_thresholds()
        if case == "shard":
            ctx.set_shard(0, 2)
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 0 and info["k1_half_tiles_separated"] == 0
        assert info["has_ties"] == (1 if case == "ties" else 0)
        if case == "shard":
            # half of the work units, nothing exchanged: the partial table is the identity order's partial table
            assert 0 < info["tiles_owned"] < info["tiles_total"]
            partial = ctx.get_codes(0, G, 0, G)
            monkeypatch.setenv("REO_K1_SLOTS", "0")
            ctx0, _, _ = _setup(pkg, X, group, seed)
            monkeypatch.delenv("REO_K1_SLOTS")
            with ctx0:
                ctx0.set_shard(0, 2)
                ctx0.build_pairs(0)
                assert np.array_equal(partial, ctx0.get_codes(0, G, 0, G)), "the shard's part of the table differs from the identity order's"
            ctx.set_shard(0, 1)
            ctx.build_pairs(0)
            assert ctx.info()["k1_slot_order"] == 1   # (the same context, unsharded: slot order again)
        code = oracle.build_codes(Xf, gid, ng, 0, thr[:, 0].tolist(), seed)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), code)


@pytest.mark.parametrize("G,S,Gp", [(33000, 64, 33792), (62000, 32, 62464)])
def test_16_planes_sampled_blocks(pkg, oracle, monkeypatch, G, S, Gp):
    """32 768 < G <= 65 535: the 16-plane loop in slot order.  Sampled blocks -- first and last rows and columns, the diagonal, the padded
    tail -- against the identity order's build and against the oracle's counts with the thresholds.  33 000 genes: two table rows per
    workgroup of the column un-permute; 62 000 (Gp above 61 440): one."""
    seed = 13
    X = pkg.synth.t0_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    blocks = [(0, 48, 0, 256), (0, 32, G - 256, G), (G - 40, G, 0, 128), (G - 64, G, G - 64, G), (16000, 16040, 16000, 16200), (20000, 20032, 300, 428),
              (5000, 5032, 29000, 29128)]
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    ctx, gid, ng = _setup(pkg, X, group, seed)
    Xf = np.asfortranarray(X.astype(np.float64))
    with ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] > 0 and info["Gp"] == Gp
        got = [ctx.get_codes(*b) for b in blocks]
    for b, g in zip(blocks[:4], got[:4]):
        assert np.array_equal(g, _expected_block_codes(oracle, Xf, gid, thr, seed, *b)), b
    for b, g, w in zip(blocks, got, _identity_codes(pkg, X, group, seed, monkeypatch, blocks)):
        assert np.array_equal(g, w), b


def test_info_after_another_matrix_on_the_same_context(pkg, oracle, monkeypatch):
    """The count of separated items is taken over what the LAST build left.  A context that has built in slot order and then gets a
    larger matrix (another padded gene count, ranked again by pair_counts, no table built yet) has no such build: info() reads 0 for
    both fields and counts nothing; the next build counts its own items; a failed set_matrix leaves nothing behind either."""
    seed = 7
    monkeypatch.delenv("REO_K1_SLOTS", raising=False)
    X1 = pkg.synth.t0_ranks(1000, 64, seed)
    X2 = pkg.synth.t0_ranks(2049, 66, seed)
    ctx, gid, ng = _setup(pkg, X1, pkg.synth.groups(64), seed)
    with ctx:
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] == 152 and info["Gp"] == 1024
        ctx.set_matrix(X2)
        assert ctx.info()["k1_slot_order"] == 0 and ctx.info()["k1_half_tiles_separated"] == 0
        gid2, lev2 = pkg.encode_groups(pkg.synth.groups(66))
        ctx.set_groups(gid2, 2)
        ctx.compute_thresholds(0.01)
        gt, eq = ctx.pair_counts(0, 8, 2000, 2049)             # ranks the new matrix: the context's geometry is the larger one now
        egt, eeq = oracle.pair_counts(np.asfortranarray(X2.astype(np.float64)), gid2, 2, 0, 8, 2000, 2049)
        assert np.array_equal(gt, egt) and np.array_equal(eq, eeq)
        info = ctx.info()
        assert info["Gp"] == 3072 and info["k1_slot_order"] == 0 and info["k1_half_tiles_separated"] == 0
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["k1_half_tiles_separated"] == 970
        ctx.set_matrix(X1)                                      # back to the small one: again nothing until it is built
        assert ctx.info()["k1_slot_order"] == 0 and ctx.info()["k1_half_tiles_separated"] == 0


def test_end_to_end_equal_with_and_without_slots(pkg, monkeypatch):
    """identify_degs at 2 049 x 66, 16 forced passes: result, trace and iteration count identical under REO_K1_SLOTS=1 and 0."""
    G, S, seed = 2049, 66, 7
    X = pkg.synth.t0_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 300, seed)
    out = {}
    for slots in ("1", "0"):
        monkeypatch.setenv("REO_K1_SLOTS", slots)
        ctx, gid, ng = _setup(pkg, X, group, seed)
        with ctx:
            ctx.build_pairs(0)
            assert ctx.info()["k1_slot_order"] == int(slots)
            out[slots] = ctx.identify_degs(ref0, 1.0, 0.05, 16, 0)
    (r1, i1, t1), (r0, i0, t0) = out["1"], out["0"]
    assert i1 == i0 == 16
    assert np.array_equal(np.asarray(t1), np.asarray(t0), equal_nan=True)
    assert np.array_equal(r1, r0, equal_nan=True)
