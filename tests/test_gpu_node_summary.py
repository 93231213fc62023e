"""The node summary of the descent: a node record keeps the pick of the node's
first UCB scan (Ns = 0), found in the expansion's P-write pass, so that scan reads neither P nor
the edge slots.  The pick must be the full scan's, bit for bit: the same trees, records and stream
counters with YK_NODE_SUMMARY=0 (every interior level a full scan) and with the default."""
import numpy as np
import pytest

from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import yacht_amd
    from yacht_amd import engine, nnet
    return yacht_amd, engine, nnet


@pytest.fixture(scope="module")
def net(Y):
    _, _, N = Y
    return N.YkNet(spec.closed_form_weights(256, 6), 256, 6)


def _run(E, n, sims, prior, net, seed, base, **kw):
    eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net if prior == "net" else None, prior=prior, max_moves=48, **kw)
    eng.run(seed, base)
    st = eng.stats()
    rec = eng.records()
    eng.close()
    assert st["errors"] == 0, st
    return rec, st


@pytest.mark.parametrize("prior,sims,env", [
    ("hash", 40, {}),
    ("net", 25, {}),
    ("hash", 200, {}),                      # deep trees, many revisited nodes
    ("hash", 60, {}),
    ("net", 40, {}),
    ("hash", 60, {"YK_ROOT_SCAN": "0"}),    # the roots too go through the summary
])
def test_node_summary_equals_full_scan(Y, net, prior, sims, env, monkeypatch):
    """A node's first scan takes the record's stored pick (the argmax of (c P) sqe0 in the scan's own
    f32 operations, lowest index among equals); every later scan of the node is the full scan.
    Identical records and counters either way, and fewer entries read."""
    _, E, _ = Y
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = []
    for mode in ("0", "1"):
        monkeypatch.setenv("YK_NODE_SUMMARY", mode)
        out.append(_run(E, 192, sims, prior, net, 707, 900))
    (r0, s0), (r1, s1) = out
    print(f"scanned: full {s0['scanned']}, summary {s1['scanned']}; expansions {s0['expansions']}")
    assert s1["expansions"] == s0["expansions"] and s1["path_edges"] == s0["path_edges"]
    assert s1["scan_edges"] == s0["scan_edges"]  # a first scan gathers no edge either way
    for k in FIELDS:
        assert np.array_equal(r1[k], r0[k]), k
    assert s1["scanned"] < s0["scanned"]


def test_node_summary_two_groups_equal_one(Y, net, monkeypatch):
    """Two game groups on their own streams, the summary on: the records of one group."""
    _, E, _ = Y
    monkeypatch.delenv("YK_NODE_SUMMARY", raising=False)
    (r1, s1), (r2, s2) = (_run(E, 32, 25, "net", net, 515, 300, groups=g) for g in (1, 2))
    assert s1["groups"] == 1 and s2["groups"] == 2
    assert s2["expansions"] == s1["expansions"]
    for k in FIELDS:
        assert np.array_equal(r2[k], r1[k]), k
