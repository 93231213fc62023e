"""Search-value targets, the parts that need no GPU: the fixture recorded from
the reference's own Nsa / Qsa agrees with the restatement in tests/value_ref.py, the restatement obeys the
identities the definition implies, the word encoding round-trips, the header, the binding and the library
agree on the new field and entry point, and bad knobs are rejected before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import value_ref as V
from conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "root_values_hash.npz"))


def _triples(fx, i, j):
    a0, a1 = int(fx["triple_off"][i, j]), int(fx["triple_off"][i, j + 1])
    return list(zip(fx["triple_action"][a0:a1], fx["triple_n"][a0:a1], fx["triple_q"][a0:a1]))


def _games(fx):
    for i in range(len(fx["n_moves"])):
        T = int(fx["n_moves"][i])
        yield fx["q64"][i, :T].astype(np.float32), fx["values"][i, :T], fx["players"][i, :T], T


# ------------------------------------------------------------------ the fixture
def test_fixture_root_values_are_the_restatement(fx):
    n = 0
    for i in range(len(fx["n_moves"])):
        for j in range(int(fx["n_moves"][i])):
            tr = _triples(fx, i, j)
            assert [int(t[0]) for t in tr] == sorted(int(t[0]) for t in tr)
            q = V.root_value(tr)
            assert q.dtype == np.float64 and q.tobytes() == fx["q64"][i, j].tobytes(), (i, j)
            n += len(tr)
    assert n == len(fx["triple_q"]) > 2000


def test_fixture_counts_are_the_episode_fixture(fx, golden):
    ep = golden("episodes_hash.npz")
    assert np.array_equal(fx["meta"], ep["meta"][:, :5]) and np.array_equal(fx["cpuct"], ep["cpuct"])
    assert np.array_equal(fx["n_moves"], ep["meta"][:, 4])
    assert np.array_equal(fx["triple_off"], ep["count_off"])
    assert np.array_equal(fx["triple_action"], ep["count_action"])
    assert np.array_equal(fx["triple_n"], ep["count_n"])
    T = ep["moves"].shape[1]
    assert np.array_equal(fx["players"][:, :T], ep["moves"][:, :, 1])
    assert np.array_equal(fx["values"], ep["values"])


def test_fixture_root_values_lie_in_the_unit_interval(fx):
    for i in range(len(fx["n_moves"])):
        q = fx["q64"][i, :int(fx["n_moves"][i])]
        assert np.all(np.isfinite(q)) and np.all(np.abs(q) <= 1.0)
    assert (fx["triple_n"] > 0).all()  # the reference creates an Nsa entry with its first visit


# ------------------------------------------------------------------ identities on the fixture's games
def test_off_is_the_outcome(fx):
    for q, z, p, T in _games(fx):
        got = V.value_targets(np.full(T, np.nan, np.float32), z, p, T, 0.0, 1.0)  # reads no q
        assert np.array_equal(got.view(np.uint32), z.astype(np.float32).view(np.uint32))


def test_full_mix_is_the_root_value(fx):
    for q, z, p, T in _games(fx):
        for lam in (1.0, 0.5):
            assert np.array_equal(V.value_targets(q, z, p, T, 1.0, lam), q)


def test_td0_is_the_next_root_value_from_the_movers_side(fx):
    for q, z, p, T in _games(fx):
        got = V.value_targets(q, z, p, T, 0.0, 0.0)
        want = np.empty(T, dtype=np.float32)
        want[:-1] = (p[:-1] * p[1:]).astype(np.float32) * q[1:]
        want[-1] = np.float32(z[-1])
        assert np.array_equal(got, want)


@pytest.mark.parametrize("beta", [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("lam", [0.0, 0.8, 0.95, 1.0])
def test_targets_stay_in_the_unit_interval(fx, beta, lam):
    """|W|, |Z| <= 1, so by induction |G_t| <= 1: each rounded product is bounded by its coefficient
    (rounding is monotone and the coefficient is representable), 1 - lam is exact for lam in [0.5, 1], and
    the rounded sum of two numbers whose exact sum is <= 1 cannot exceed 1.  Likewise |v|."""
    for q, z, p, T in _games(fx):
        v = V.value_targets(q, z, p, T, beta, lam)
        assert np.all(np.isfinite(v)) and np.all(np.abs(v) <= 1.0)


def test_hand_worked_case():
    """Three moves, players (+1, +1, -1), q = (0.5, -0.25, 0.75), final result -1 for player +1, so
    z = (-1, -1, +1); beta = 0.25, lambda = 0.5 (every number below is exact in binary).
      W = p q = (0.5, -0.25, -0.75) ;  Z = p z = (-1, -1, -1)
      G_2 = Z_2 = -1
      G_1 = 0.5 W_2 + 0.5 G_2 = -0.375 - 0.5 = -0.875
      G_0 = 0.5 W_1 + 0.5 G_1 = -0.125 - 0.4375 = -0.5625
      target = p G = (-0.5625, -0.875, 1)
      v = 0.75 target + 0.25 q = (-0.421875 + 0.125, -0.65625 - 0.0625, 0.75 + 0.1875)
        = (-0.296875, -0.71875, 0.9375)"""
    q = np.array([0.5, -0.25, 0.75], dtype=np.float32)
    z = np.array([-1.0, -1.0, 1.0])
    p = np.array([1, 1, -1])
    assert V.value_targets(q, z, p, 3, 0.25, 0.5).tolist() == [-0.296875, -0.71875, 0.9375]
    assert V.value_targets(q, z, p, 3, 0.0, 0.5).tolist() == [-0.5625, -0.875, 1.0]
    assert V.value_targets(q, z, p, 3, 0.0, 0.0).tolist() == [-0.25, -0.75, 1.0]  # p_t p_{t+1} q_{t+1}, then z
    assert V.value_targets(q, z, p, 3, 0.0, 1.0).tolist() == [-1.0, -1.0, 1.0]
    assert V.root_value([(3, 1, 0.5), (7, 3, -0.25), (9, 0, 1.0)]) == (0.5 - 0.75) / 4.0
    w = np.array([0, 5, 0], dtype=np.uint32)
    assert V.needs_missing(w, 3, 0.5, 1.0).tolist() == [True, False, True]
    assert V.needs_missing(w, 3, 0.0, 0.5).tolist() == [True, True, False]
    assert not V.needs_missing(w, 3, 0.0, 1.0).any()


# ------------------------------------------------------------------ the word
def test_word_encoding():
    assert V.encode(np.float32(0.0)) == 0x80000000 and V.encode(np.float32(-0.0)) == 0x80000000
    assert np.isnan(V.decode(np.uint32(0)))
    assert V.decode(np.uint32(0x80000000)).tobytes() == np.float32(-0.0).tobytes()
    rng = np.random.RandomState(3)
    bits = np.concatenate([rng.randint(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32),
                           np.array([1, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000, 0x7FC00000, 0x00800000,
                                     0x80000001, 0xFFFFFFFF], dtype=np.uint32)])
    bits = bits[(bits << np.uint32(1)) != 0]  # every float32 but the two zeros
    words = V.encode(bits.view(np.float32))
    assert (words != 0).all() and np.array_equal(words, bits)
    assert np.array_equal(V.decode(words).view(np.uint32), bits)
    from yacht_amd.engine import decode_root_values
    both = np.concatenate([bits, np.array([0], dtype=np.uint32)])
    assert np.array_equal(decode_root_values(both.view(np.int32)).view(np.uint32), V.decode(both).view(np.uint32))


# ------------------------------------------------------------------ ABI
def _header():
    src = open(os.path.join(REPO, "include", "yacht_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_field_and_the_entry_point():
    src = _header()
    assert re.search(r"\byk_examples_value_targets\s*\(", src)
    body = re.search(r"typedef struct \{([^}]*)\}\s*yk_engine_config_t;", src).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields[-1] == "int record_root_values"
    assert fields[-3:-1] == ["double dirichlet_alpha", "double dirichlet_eps"]  # appended: offsets kept


def test_binding_mirrors_the_struct():
    from yacht_amd import _lib
    S = _lib.YkEngineConfigFull
    names = [f[0] for b in (_lib.YkEngineConfig, S) for f in b._fields_]
    assert names[-1] == "record_root_values" and S.record_root_values.offset == 80 and C.sizeof(S) == 88
    assert dict(S._fields_)["record_root_values"] is C.c_int
    assert S.dirichlet_alpha.offset == 64 and S.n_envs.offset == 0
    # the header's fields, in order, are the binding's
    body = re.search(r"typedef struct \{([^}]*)\}\s*yk_engine_config_t;", _header()).group(1)
    assert [f.split()[-1] for f in body.split(";") if f.strip()] == names
    assert _lib.SIGNATURES["yk_examples_value_targets"] == (
        [C.c_void_p] + [C.c_int] * 4 + [C.c_int64] * 3 + [C.c_double] * 2 + [C.c_void_p] * 4)
    import inspect
    from yacht_amd import engine, replay
    assert inspect.signature(engine.SelfPlayEngine.__init__).parameters["record_root_values"].default is False
    sig = inspect.signature(replay.examples_from_images).parameters
    assert sig["value_mix"].default == 0.0 and sig["value_lambda"].default == 1.0


def test_library_exports_the_entry_point():
    import yacht_amd
    assert hasattr(C.CDLL(yacht_amd.LIB_PATH), "yk_examples_value_targets")


# ------------------------------------------------------------------ argument checks, no device call
BAD = [(-0.1, 1.0), (1.5, 1.0), (float("nan"), 1.0), (0.0, -0.1), (0.0, 1.5), (0.0, float("nan"))]


@pytest.mark.parametrize("beta,lam", BAD)
def test_c_entry_point_rejects_bad_knobs_without_a_gpu(beta, lam):
    import yacht_amd
    lib = yacht_amd.lib()
    buf = (C.c_char * 64)()  # (never read: the knobs are checked first)
    miss = C.c_int64(-7)
    args = (C.addressof(buf), 1, 1, 1, 1, -1, 0, 0)
    assert lib.yk_examples_value_targets(*args, beta, lam, None, None, C.byref(miss), None) == -1
    assert miss.value == -7


def test_c_entry_point_rejects_bad_shapes_without_a_gpu():
    import yacht_amd
    lib = yacht_amd.lib()
    buf = (C.c_char * 64)()
    f = lib.yk_examples_value_targets
    assert f(None, 1, 1, 1, 1, -1, 0, 0, 0.5, 0.5, None, None, None, None) == -1
    assert f(C.addressof(buf), 1, 1, 1, 1, -1, 0, -1, 0.5, 0.5, None, None, None, None) == -1  # n_examples < 0
    assert f(C.addressof(buf), 1, 1, 1, 1, -1, 0, 4, 0.5, 0.5, None, None, None, None) == -1  # NULL values


def test_reloaded_history_trains_on_outcomes_with_one_warning(tmp_path, caplog):
    """A resumed run starts whatever the knobs: the examples file holds outcomes only, and loading it with
    non-default knobs logs one warning (none with the defaults)."""
    import logging
    import shutil

    from yacht_amd import examples_io as X
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    hist = X.load_reference_examples(os.path.join(GOLDEN, "examples_ref.pkl"))
    shutil.copy(os.path.join(GOLDEN, "examples_ref.pkl"), tmp_path / "best.pth.tar.examples")
    for extra, warnings in ((dict(valueMix=0.5), 1), (dict(valueLambda=0.9), 1), ({}, 0),
                            (dict(valueMix=0.0, valueLambda=1.0), 0)):
        args = dotdict(numMCTSSims=4, cpuct=1.5, tempThreshold=15, load_folder_file=(str(tmp_path), "best.pth.tar"),
                       **extra)
        c = Coach(YachtGame(seed=1, env_id=0), object(), args)
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="yacht_amd.coach"):
            c.loadTrainExamples()
        assert [len(it) for it in c.trainExamplesHistory] == [len(it) for it in hist] and c.skipFirstSelfPlay
        got = [r for r in caplog.records if r.levelno == logging.WARNING]
        assert len(got) == warnings
        assert all("outcomes" in r.getMessage() for r in got)


@pytest.mark.parametrize("beta,lam", BAD)
def test_python_layers_reject_bad_knobs_before_any_device_call(beta, lam):
    from yacht_amd import replay
    from yacht_amd.coach import Coach
    from yacht_amd.utils import dotdict
    with pytest.raises(ValueError, match="value_mix|value_lambda"):
        replay.examples_from_images(None, 4, 48, 8, value_mix=beta, value_lambda=lam)  # (images never touched)
    with pytest.raises(ValueError, match="value_mix|value_lambda"):
        Coach(None, None, dotdict(numMCTSSims=4, cpuct=1.5, tempThreshold=15, valueMix=beta, valueLambda=lam))
