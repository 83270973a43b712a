"""PQ training on the GPU at its edges, byte-identical to the oracle (O.pq_train, OraclePQ.refine, serialize) for the same seed.

A k-means round assigns the points either through the encode kernel (`fast`: uniform sub-vectors of size 2, 4, 6, 8, 12 or 16 and 256
clusters, assign_points in pq_train.cpp) or through km_assign (`plain`: everything else, or JVECTOR_HIP_KM_ASSIGN_PLAIN=1, read at
each round).  Every case here runs in both modes: fast == plain == oracle.  The CPU twins of the degenerate inputs (small n,
identical points, refine on a handful of points, anisotropic sizes) are in tests/test_pq_train_emulated.py, which runs km_assign:
a failure here that has no twin failure there lies in the launch or encode path, not in the kernel bodies."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from oracle import oracle as O

ASSIGN = [pytest.param(False, id="default"), pytest.param(True, id="km_assign")]


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


@pytest.fixture
def assign(monkeypatch):
    def set_mode(plain):
        if plain:
            monkeypatch.setenv("JVECTOR_HIP_KM_ASSIGN_PLAIN", "1")
        else:
            monkeypatch.delenv("JVECTOR_HIP_KM_ASSIGN_PLAIN", raising=False)
    return set_mode


def data(n, D, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((40, D)).astype(np.float32)
    return (centers[rng.integers(0, 40, n)] + 0.3 * rng.standard_normal((n, D))).astype(np.float32)


def both_modes(assign, fn):
    """fn() under the default assignment and under km_assign -> the two results"""
    out = []
    for plain in (False, True):
        assign(plain)
        out.append(fn())
    return out


# ------------------------------------------------------------------------------------------------
# every assignment path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M,path", [(4, 2, "fast-2"), (8, 2, "fast-4"), (12, 2, "fast-6"), (24, 2, "fast-12"), (32, 2, "fast-16"),
                                      (3, 3, "plain-1"), (6, 2, "plain-3"), (10, 2, "plain-5"), (128, 2, "plain-64-replay")])
def test_every_assignment_path(ctx, assign, D, M, path):
    assert int(path.split("-")[1]) == D // M
    v = data(2000, D, D)
    x = data(1500, D, D + 1)
    want, _ = O.pq_train(v, M, globally_center=True, seed=7)
    want_blob, want_refined = want.serialize(6), want.refine(x, 2, seed=3).serialize(6)
    assert want_refined != want_blob
    for plain, pq in zip((False, True), both_modes(assign, lambda: J.ProductQuantization.compute(ctx, v, M, globally_center=True, seed=7))):
        assert pq.write(6) == want_blob, f"km_assign={plain}"
        assign(plain)
        assert pq.refine(x, 2, seed=3).write(6) == want_refined, f"km_assign={plain}"


def test_sub_vectors_longer_than_64(ctx):
    with pytest.raises(ValueError):
        J.ProductQuantization.compute(ctx, data(300, 130, 1), 2)


# ------------------------------------------------------------------------------------------------
# early stop and empty clusters
# ------------------------------------------------------------------------------------------------
def test_early_stop_per_subspace_and_empty_clusters(ctx, assign):
    """the inputs of test_pq_train_emulated.py's test of the same name, on the device, where this shape (three sub-vectors of 8) assigns
    through the encode kernel: subspace 0 stops early, subspace 1 has 100 distinct sub-vectors (156 clusters run empty every round and
    are re-seeded from the RNG stream), subspace 2 runs all six rounds"""
    D, M = 24, 3
    rng = np.random.default_rng(5)
    v = np.empty((4000, D), np.float32)
    v[:, :8] = rng.standard_normal((300, 8)).astype(np.float32)[rng.integers(0, 300, 4000)]
    v[:, 8:16] = rng.standard_normal((100, 8)).astype(np.float32)[rng.integers(0, 100, 4000)]
    v[:, 16:] = rng.standard_normal((4000, 8)).astype(np.float32)
    want, rounds = O.pq_train(v, M, globally_center=False, seed=2)
    assert rounds[0] < rounds[2] == 6
    assert len(np.unique(want.encode_all(v)[:, 1])) <= 100
    for plain, pq in zip((False, True), both_modes(assign, lambda: J.ProductQuantization.compute(ctx, v, M, seed=2))):
        assert pq.write(6) == want.serialize(6), f"km_assign={plain}"


# ------------------------------------------------------------------------------------------------
# small and awkward n
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 257, 300, 321])
def test_small_n(ctx, assign, n):
    """n == k; one point more; a partial last 64-lane block in km_pp_init (300 = 4 * 64 + 44, 321 = 5 * 64 + 1)"""
    v = data(n, 8, n)
    want, _ = O.pq_train(v, 2, globally_center=True, seed=4)
    assert np.isfinite(want.codebooks).all()
    for plain, pq in zip((False, True), both_modes(assign, lambda: J.ProductQuantization.compute(ctx, v, 2, globally_center=True, seed=4))):
        assert pq.write(6) == want.serialize(6), f"km_assign={plain}"


def test_fewer_points_than_clusters(ctx):
    with pytest.raises(ValueError):
        J.ProductQuantization.compute(ctx, data(255, 8, 1), 2)


def test_identical_points(ctx, assign):
    """300 copies of one point: the k-means++ draw sees a total distance of 0, 255 clusters run empty in every round and the oracle
    runs all six"""
    v = np.repeat(data(1, 8, 3), 300, axis=0)
    want, rounds = O.pq_train(v, 2, seed=6)
    assert list(rounds) == [6, 6] and np.isfinite(want.codebooks).all()
    for plain, pq in zip((False, True), both_modes(assign, lambda: J.ProductQuantization.compute(ctx, v, 2, seed=6))):
        assert pq.write(6) == want.serialize(6), f"km_assign={plain}"


@pytest.mark.parametrize("repeat", [1, 10])
def test_perfect_reconstruction(ctx, assign, repeat):
    """TestProductQuantization.testPerfectReconstruction (:54-80) trained on the device: as many distinct integer 3-d points as
    clusters, then each repeated ten times; every vector decodes to itself"""
    rng = np.random.default_rng(42)
    v = np.repeat(rng.integers(0, 100000, (256, 3)).astype(np.float32), repeat, axis=0)
    want, _ = O.pq_train(v, 2, seed=5)
    for plain, pq in zip((False, True), both_modes(assign, lambda: J.ProductQuantization.compute(ctx, v, 2, seed=5))):
        blob = pq.write(6)
        assert blob == want.serialize(6), f"km_assign={plain}"
        got = O.OraclePQ.parse(blob)[0]
        codes = pq.encode_all(v)
        assert np.array_equal(np.stack([got.decode(c) for c in codes]), v)


# ------------------------------------------------------------------------------------------------
# refine at its edges
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(ctx):
    v = data(2000, 8, 8)
    want, _ = O.pq_train(v, 2, globally_center=True, seed=7)
    pq = J.ProductQuantization.compute(ctx, v, 2, globally_center=True, seed=7)
    assert pq.write(6) == want.serialize(6)
    return pq, want


@pytest.mark.parametrize("plain", ASSIGN)
@pytest.mark.parametrize("n,rounds", [(40, 1), (1, 2), (40, 0)])
def test_refine_on_fewer_points_than_clusters(ctx, assign, trained, n, rounds, plain):
    assign(plain)
    pq, want = trained
    x = data(n, 8, 100 + n)
    blob = pq.refine(x, rounds, seed=3).write(6)
    assert blob == want.refine(x, rounds, seed=3).serialize(6)
    assert (blob == want.serialize(6)) == (rounds == 0)      # no round: the codebooks as they were


@pytest.mark.parametrize("plain", ASSIGN)
def test_refine_50_clusters_on_30_points(ctx, assign, plain):
    assign(plain)
    v = data(1000, 8, 50)
    want, _ = O.pq_train(v, 2, k=50, seed=5)
    pq = J.ProductQuantization.compute(ctx, v, 2, cluster_count=50, seed=5)
    assert pq.write(6) == want.serialize(6)
    x = data(30, 8, 51)
    pq2 = pq.refine(x, 2, seed=3)
    assert pq2.get_cluster_count() == 50 and pq2.write(6) == want.refine(x, 2, seed=3).serialize(6)


def test_refine_negative_rounds(ctx, trained):
    with pytest.raises(ValueError):
        trained[0].refine(data(40, 8, 1), -1)


# ------------------------------------------------------------------------------------------------
# anisotropic sizes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M,T", [(4, 2, 0.2), (10, 3, 0.2), (32, 2, 0.5)])
def test_anisotropic_sizes(ctx, assign, D, M, T):
    """sub-vectors of 2, of 4 / 3 / 3 and of 16 dimensions (the existing tests have 8): six unweighted rounds — fast assignment at sizes
    2 and 16 — then six anisotropic ones"""
    v = data(800, D, D + 7)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    want, _ = O.pq_train(v, M, seed=9, anisotropic_threshold=T)
    assert np.isfinite(want.codebooks).all()
    assert not np.array_equal(want.codebooks, O.pq_train(v, M, seed=9)[0].codebooks)
    for plain, pq in zip((False, True), both_modes(assign, lambda: J.ProductQuantization.compute(ctx, v, M, seed=9, anisotropic_threshold=T))):
        blob = pq.write(6)
        got, ver, aniso, used = O.OraclePQ.parse(blob)
        assert used == len(blob) and ver == 6 and aniso == np.float32(T)
        assert np.array_equal(got.codebooks, want.codebooks), f"km_assign={plain}"
        assert blob == want.serialize(6, aniso=T)


@pytest.mark.parametrize("D,M", [(34, 2), (3, 2), (4, 4)])
def test_anisotropic_size_limits(ctx, D, M):
    """sub-vectors of 17 dimensions; D / M < 2"""
    v = data(400, D, 1)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    with pytest.raises(ValueError):
        J.ProductQuantization.compute(ctx, v, M, anisotropic_threshold=0.2)
