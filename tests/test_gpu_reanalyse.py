"""Reanalysis on the GPU: yk_reanalyse_select, yk_policies_from_counts and
yk_policies_splice equal tests/reanalyse_ref.py bit for bit; a reanalysed move-0 example under its game's own
stream and counter is the stored example again; a reanalysed row is what the MCTS plugin's getActionProb
returns for that board; the result does not depend on the chunking; and the Coach's knob refreshes the older
iterations of the window and nothing else.  Off by default, and then unobservable."""
import ctypes as C

import numpy as np
import pytest

import reanalyse_ref as RR
import sample_ref as SR
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A = RR.A
SEED, BASE, SIMS, CPUCT = 29, 700, 12, 1.5


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import yacht_amd
    from yacht_amd import engine, kernels, replay
    return yacht_amd, engine, kernels, replay


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) and g.dtype == w.dtype for g, w in zip(got, want))


def _host(csr):
    return tuple(t.cpu().numpy() for t in csr)


def _dev(csr):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in csr)


def _rows(csr):
    ip, cols, vals = csr
    return [(cols[ip[i]:ip[i + 1]].tolist(), _bits(vals[ip[i]:ip[i + 1]]).tolist()) for i in range(len(ip) - 1)]


# ------------------------------------------------------------------ 1. select
_U = {}


N_BIG = 256 * 1024 + 1  # 1025 blocks of 256 rows: thread 0 of the scan's middle pass owns two block sums


def _uniforms(base):
    if base not in _U:
        # the numpy Philox of tests/sample_ref.py in this domain, held to the restatement over the first 4096
        _U[base] = SR.uniforms(SEED, 5, base, N_BIG, domain=RR.DOMAIN)
        assert np.array_equal(_U[base][:4096], np.asarray([RR.uniform(SEED, 5, base + i) for i in range(4096)]))
    return _U[base]


@pytest.mark.parametrize("base", [0, 2**32 - 3])  # (the second crosses counter word 0 into word 1)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, N_BIG])
def test_select_is_the_restatement(Y, n, base):
    from yacht_amd._lib import YK_ERR_CAPACITY
    lib, K = Y[0].lib(), Y[2]
    if n == 257:  # the cached uniforms are the restatement's
        assert np.array_equal(RR.select(n, base, SEED, 5, 0.25), np.nonzero(_uniforms(base)[:n] < 0.25)[0])
    for f in (0.0, 0.25, 1.0):
        want = np.nonzero(_uniforms(base)[:n] < f)[0].astype(np.int32)
        got = K.reanalyse_select(n, SEED, 5, f, index_base=base)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (n, base, f)
        assert K.reanalyse_select(n, SEED, 5, f, index_base=base, count_only=True) == len(want)
        if len(want):  # a capacity one short: the error, the count still reported, nothing past the capacity written
            buf = torch.full((len(want) + 1,), -9, dtype=torch.int32, device="cuda")
            m = C.c_int64()
            rc = lib.yk_reanalyse_select(n, base, SEED, 5, f, buf.data_ptr(), len(want) - 1, C.byref(m), None)
            assert rc == YK_ERR_CAPACITY and m.value == len(want)
            assert buf[len(want) - 1:].tolist() == [-9, -9]
    assert len(K.reanalyse_select(n, SEED, 5, 0.0, index_base=base)) == 0
    assert K.reanalyse_select(n, SEED, 5, 1.0, index_base=base).tolist() == list(range(n))


# ------------------------------------------------------------------ 2. from counts
def _crafted():
    rng = np.random.default_rng(7)
    c = np.zeros((40, A), dtype=np.int32)
    c[0, 1234] = 3                                   # a single entry
    c[1, [0, 3225]] = [2, 5]                         # the two ends
    c[2, [63, 64, 65, 2000]] = [9, 11, 11, 11]       # a tie at the maximum: the lowest wins
    c[3, rng.choice(A, size=3024, replace=False)] = rng.integers(1, 50, size=3024)  # a row of 3024 entries
    # row 4: all zero
    c[5, [7, 8, 9]] = [-4, 6, -1]                    # negative counts are not entries
    c[6, [10, 700, 3000]] = [65536, 70000, 2**31 - 1]  # counts above 65535
    c[7, :] = 2**31 - 1                              # the largest sum: 3226 (2^31 - 1) < 2^43
    c[8, [5, 6]] = [-7, -7]                          # only negative counts: empty
    c[9, [127, 128, 191, 192]] = 1                   # a tie of ones across the lanes' 64-column groups
    for r in range(10, 40):                          # random sparse rows
        k = int(rng.integers(1, 90))
        c[r, rng.choice(A, size=k, replace=False)] = rng.integers(1, 40, size=k)
    return c


def test_from_counts_is_the_restatement(Y):
    K = Y[2]
    c = _crafted()
    want = RR.from_counts(c)
    assert want[4] == 2 and want[3][[2, 4, 5, 6, 7, 8, 9]].tolist() == [64, -1, 8, 3000, 0, -1, 127]
    pol, tg, n_empty = K.policies_from_counts(torch.from_numpy(c).to("cuda"))
    assert _same(_host(pol), want[:3])
    assert np.array_equal(tg.cpu().numpy(), want[3]) and n_empty == want[4]
    # one row and no row
    one = K.policies_from_counts(torch.from_numpy(c[3:4]).to("cuda"))
    assert _same(_host(one[0]), RR.from_counts(c[3:4])[:3]) and one[2] == 0
    none = K.policies_from_counts(torch.zeros((0, A), dtype=torch.int32, device="cuda"))
    assert none[0][0].tolist() == [0] and none[0][1].numel() == 0 and none[2] == 0
    # 1030 rows: more than one block of the row scan's second pass
    rng = np.random.default_rng(8)
    big = np.zeros((1030, A), dtype=np.int32)
    for r in range(1030):
        k = int(rng.integers(0, 5))
        big[r, rng.choice(A, size=k, replace=False)] = rng.integers(1, 9, size=k)
    wb = RR.from_counts(big)
    pb, tb, eb = K.policies_from_counts(torch.from_numpy(big).to("cuda"))
    assert _same(_host(pb), wb[:3]) and np.array_equal(tb.cpu().numpy(), wb[3]) and eb == wb[4] > 0


def _play(Y, temp_threshold):
    _, E, _, R = Y
    eng = E.SelfPlayEngine(8, SIMS, CPUCT, temp_threshold, prior="hash", max_moves=48)
    eng.run(SEED, BASE)
    st, rec, img = eng.stats(), eng.records(), eng.pack_records()
    eng.close()
    assert st["errors"] == 0 and (rec["n_moves"] == 48).all()
    shard = R.examples_from_images(img.reshape(1, -1), 8, 48, SIMS)
    assert len(shard) == 8 * 48
    return rec, shard


@pytest.fixture(scope="module")
def games(Y):
    """8 hash-prior games, tempThreshold 48: (records, the shard of their examples).  Moves 0 .. 46 are played
    at temperature 1; the reference's temp = int(episodeStep < tempThreshold) counts the steps from 1
    (Coach.py:59-61), so the 48th move is a temp-0 move and its stored row a one-hot."""
    rec, shard = _play(Y, 48)
    assert (rec["info"][:, :47, 0] == 1).all() and (rec["info"][:, 47, 0] == 0).all()
    return rec, shard


def _dense_visits(rec):
    dense = np.zeros((8 * 48, A), dtype=np.int32)
    off = rec["visits_off"]
    for k in range(8 * 48):
        for a, c in rec["visits"][off[k]:off[k + 1]]:
            dense[k, a] = c
    return torch.from_numpy(dense).to("cuda")


def test_recorded_visits_give_the_shards_own_rows(Y, games):
    K = Y[2]
    # tempThreshold 49: every one of the 48 moves is a temp-1 move, and the whole CSR is the shard's own
    rec, shard = _play(Y, 49)
    assert (rec["info"][:, :, 0] == 1).all()
    pol, tg, n_empty = K.policies_from_counts(_dense_visits(rec))
    P = shard.policies
    assert _same(_host(pol), _host((P["pi_indptr"], P["pi_cols"], P["pi_vals"])))
    assert torch.equal(tg, shard.targets) and n_empty == 0
    # tempThreshold 48: the same for the 47 temp-1 moves of every game; the last move's stored row is the one-hot
    # of the played action, where the counts give the visit distribution (what a reanalysed row holds)
    rec, shard = games
    pol, tg, n_empty = K.policies_from_counts(_dense_visits(rec))
    P = shard.policies
    got, own = _rows(_host(pol)), _rows(_host((P["pi_indptr"], P["pi_cols"], P["pi_vals"])))
    t1 = [k for k in range(8 * 48) if k % 48 != 47]
    assert [got[k] for k in t1] == [own[k] for k in t1] and n_empty == 0
    assert np.array_equal(tg.cpu().numpy()[t1], shard.targets.cpu().numpy()[t1])
    one = _bits(np.asarray([1.0])).tolist()
    assert all(own[k] == ([int(rec["info"][k // 48, 47, 2])], one) for k in range(47, 8 * 48, 48))


# ------------------------------------------------------------------ 3. splice
def _csr(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, size=n)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = [np.sort(rng.choice(A, size=l, replace=False)) for l in lens]
    return ip, np.concatenate(cols + [np.zeros(0, dtype=np.int64)]).astype(np.int32), rng.random(int(ip[-1]))


@pytest.mark.parametrize("n", [5, 3000])
def test_splice_is_the_restatement(Y, n):
    from yacht_amd._lib import YK_ERR_RANGE
    lib, K = Y[0].lib(), Y[2]
    rng = np.random.default_rng(n)
    old = _csr(rng, n, 0, 6)
    d_old = _dev(old)
    picks = {"none": np.zeros(0, dtype=np.int32), "all": np.arange(n, dtype=np.int32),
             "ends": np.asarray([0, n - 1], dtype=np.int32),
             "some": np.sort(rng.choice(n, size=max(n // 3, 2), replace=False)).astype(np.int32)}
    for name, idx in picks.items():
        new = _csr(rng, len(idx), 0, 12)  # rows that grow, rows that shrink, and empty ones that keep the old row
        if n == 3000 and len(idx) > 2:
            ln, lo = np.diff(new[0]), np.diff(old[0])[idx]
            assert (ln > lo).any() and ((ln < lo) & (ln > 0)).any() and (ln == 0).any()
        want = RR.splice(*old, idx, *new)
        got = _host(K.policies_splice(d_old, torch.from_numpy(idx).to("cuda"), _dev(new)))
        assert _same(got, want), name
        if name == "none":
            assert _same(got, old)
        # untouched rows (and rows whose new row is empty) are the old rows, bit for bit
        keep = sorted(set(range(n)) - {int(x) for j, x in enumerate(idx) if new[0][j + 1] > new[0][j]})
        ro, rg = _rows(old), _rows(got)
        assert all(ro[i] == rg[i] for i in keep), name
    assert _same(_host(d_old), old)  # the inputs are not modified
    # n == 5 by hand: an empty new row keeps the old one
    if n == 5:
        idx = np.asarray([1, 3, 4], dtype=np.int32)
        new = (np.asarray([0, 0, 9, 10], dtype=np.int64), np.sort(rng.choice(A, 10, replace=False)).astype(np.int32),
               rng.random(10))
        got = _rows(_host(K.policies_splice(d_old, torch.from_numpy(idx).to("cuda"), _dev(new))))
        assert got[:3] == _rows(old)[:3] and got[3:] == _rows(new)[1:]
    # idx unsorted, repeated or out of range: YK_ERR_RANGE from the device
    new = _csr(rng, 2, 1, 3)
    d_new = _dev(new)
    out_ip = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    for bad in ([3, 1], [2, 2], [0, n], [-1, 2]):
        b = torch.tensor(bad, dtype=torch.int32, device="cuda")
        nnz = C.c_int64()
        rc = lib.yk_policies_splice(d_old[0].data_ptr(), d_old[1].data_ptr(), d_old[2].data_ptr(), n, b.data_ptr(), 2,
                                    d_new[0].data_ptr(), d_new[1].data_ptr(), d_new[2].data_ptr(), out_ip.data_ptr(),
                                    None, None, 0, C.byref(nnz), None)
        assert rc == YK_ERR_RANGE, bad
        with pytest.raises(ValueError, match="ascending"):
            K.policies_splice(d_old, b, d_new)


# ------------------------------------------------------------------ 4. end to end, exact
def _policy_rows(shard, rows):
    P = shard.policies
    h = _rows(_host((P["pi_indptr"], P["pi_cols"], P["pi_vals"])))
    return [h[i] for i in rows]


def test_reanalysing_move_zero_reproduces_the_stored_example(Y, games):
    R = Y[3]
    rec, shard = games
    rows = [g * 48 for g in range(8)]
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    env = [BASE + g for g in range(8)]
    ctr = [int(rec["ctr"][g][0][0]) for g in range(8)]
    outs = []
    for chunk in (4096, 3):  # one chunk; three chunks, the last one padded
        out = R.reanalyse(shard, idx, prior="hash", sims=SIMS, cpuct=CPUCT, seed=SEED, env_ids=env, ctr=ctr,
                          chunk=chunk)
        assert out.reanalysis == dict(n=8, n_empty=0, chunks=1 if chunk > 8 else 3)
        # both paths ran run_sims on a fresh tree from the same draws: the same visits, so the same row
        assert _policy_rows(out, rows) == _policy_rows(shard, rows)
        assert torch.equal(out.targets, shard.targets) and out.targets is not shard.targets
        for k in ("pi_indptr", "pi_cols", "pi_vals", "values64"):
            assert torch.equal(out.policies[k], shard.policies[k]), k
        outs.append(out)
    assert outs[0].policies["values64"] is shard.policies["values64"] and outs[0].states is shard.states
    # from counter 0 the draws differ: some other search - valid, normalised, and the rest of the shard untouched
    other = R.reanalyse(shard, idx, prior="hash", sims=SIMS, cpuct=CPUCT, seed=SEED, env_base=BASE)
    all_rows = list(range(8 * 48))
    a, b = _policy_rows(other, all_rows), _policy_rows(shard, all_rows)
    assert [i for i in all_rows if a[i] != b[i] and i not in rows] == []
    vals, ip = other.policies["pi_vals"], other.policies["pi_indptr"]
    assert all(abs(float(vals[ip[i]:ip[i + 1]].sum()) - 1.0) < 1e-12 for i in rows)


# ------------------------------------------------------------------ 5. against the plugin
def test_reanalysed_rows_are_the_plugins_action_probabilities(Y, games):
    R = Y[3]
    from yacht_amd.game import YachtGame
    from yacht_amd.mcts import MCTS
    from yacht_amd.nnet import HashPriorNet
    from yacht_amd.utils import dotdict
    _, shard = games
    rows = [17, 48 + 24, 5 * 48 + 30, 7 * 48 + 47]  # mid-game examples (and a game's last move)
    env = [900 + j for j in range(4)]
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    out = R.reanalyse(shard, idx, prior="hash", sims=SIMS, cpuct=CPUCT, seed=SEED, env_ids=env)
    assert out.reanalysis["n_empty"] == 0
    got = _policy_rows(out, rows)
    tg = out.targets.cpu().numpy()
    for j, k in enumerate(rows):
        game = YachtGame(seed=SEED, env_id=env[j])  # the stream (SEED, env), counter 0
        board = shard[k][0]
        probs = MCTS(game, HashPriorNet(game), dotdict(numMCTSSims=SIMS, cpuct=CPUCT)).getActionProb(board, temp=1)
        nz = [a for a, p in enumerate(probs) if p != 0]
        assert got[j] == (nz, _bits(np.asarray([probs[a] for a in nz], dtype=np.float64)).tolist()), k
        assert tg[k] == int(np.argmax(probs))


# ------------------------------------------------------------------ 6. a real net
def test_real_net_chunking_and_repeat_give_the_same_bits(Y):
    _, E, _, R = Y
    from yacht_amd.nnet import YkNet
    net = YkNet(spec.closed_form_weights(64, 1), 64, 1)
    eng = E.SelfPlayEngine(4, 8, CPUCT, 15, net=net, max_moves=48, record_root_values=True)
    eng.run(SEED, 40)
    img = eng.pack_records()
    eng.close()
    shard = R.examples_from_images(img.reshape(1, -1), 4, 48, 8, value_mix=0.5, value_lambda=0.9)
    idx = torch.arange(3, 4 * 48, 10, dtype=torch.int32, device="cuda")  # 19 roots
    kw = dict(net=net, sims=8, cpuct=CPUCT, seed=SEED, env_base=3000)
    a = R.reanalyse(shard, idx, chunk=4, **kw)    # 5 chunks, the last padded by one
    b = R.reanalyse(shard, idx, chunk=16, **kw)   # 2 chunks, the last padded by 13
    c = R.reanalyse(shard, idx, chunk=16, **kw)   # again
    assert (a.reanalysis["chunks"], b.reanalysis["chunks"]) == (5, 2)
    for x in (b, c):
        assert torch.equal(a.targets, x.targets)
        for k in ("pi_indptr", "pi_cols", "pi_vals", "values64"):
            assert torch.equal(a.policies[k], x.policies[k]), k
    assert a.reanalysis["n_empty"] == 0
    # value targets keep the original search's numbers: the same tensors
    assert a.values is shard.values and a.outcomes is shard.outcomes and a.root_values is shard.root_values
    assert a.states is shard.states and a.policies["values64"] is shard.policies["values64"]
    # the new rows: one per chosen example, each a distribution over valid moves; the others untouched
    rows = idx.tolist()
    ra, rs = _policy_rows(a, range(len(shard))), _policy_rows(shard, range(len(shard)))
    assert all(ra[i] == rs[i] for i in range(len(shard)) if i not in rows)
    assert any(ra[i] != rs[i] for i in rows)  # (other draws, and the one-hot rows of temp-0 moves become distributions)
    ip, vals = a.policies["pi_indptr"], a.policies["pi_vals"]
    assert all(abs(float(vals[ip[i]:ip[i + 1]].sum()) - 1.0) < 1e-12 for i in rows)
    h = a.host()
    assert h["pi_indptr"][-1] == len(h["pi_cols"]) and np.array_equal(h["targets"], a.targets.cpu().numpy())


# ------------------------------------------------------------------ 7. Coach
ARGS = dict(numIters=2, numEps=4, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000, numMCTSSims=4,
            arenaCompare=2, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=1,
            batch_size=48, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3, amp=False)


def _learn(monkeypatch, tmp_path, name, **extra):
    from yacht_amd import replay
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    ck = str(tmp_path / name)
    torch.manual_seed(5)
    net = NNetWrapper(YachtGame(seed=21, env_id=500), dotdict(ARGS, checkpoint=ck, load_folder_file=(ck, "best.pth.tar"),
                                                             **extra))
    coach = Coach(net.game, net, net.args)
    calls = dict(streams=[], select=[], reanalyse=[])
    streams, select, reanalyse = coach._streams, replay.reanalyse_select, replay.reanalyse

    def _streams(n):
        calls["streams"].append((coach._next_env, n))
        return streams(n)

    def _select(n, seed, key, fraction, index_base=0, **kw):
        calls["select"].append((n, seed, key, fraction, index_base))
        return select(n, seed, key, fraction, index_base=index_base, **kw)

    def _reanalyse(shard, idx, **kw):
        out = reanalyse(shard, idx, **kw)
        calls["reanalyse"].append((len(coach.trainExamplesHistory), shard, idx, out, kw))
        return out
    with monkeypatch.context() as mp:
        mp.setattr(coach, "_streams", _streams)
        mp.setattr(replay, "reanalyse_select", _select)
        mp.setattr(replay, "reanalyse", _reanalyse)
        coach.learn()
    return coach, calls


def test_coach_reanalyses_the_older_iterations_only(Y, monkeypatch, tmp_path):
    off, c_off = _learn(monkeypatch, tmp_path, "off")
    # off: no selection, no reanalysis engine, and the stream ids of today - episodes, then the arena's, per iteration
    assert c_off["select"] == [] and c_off["reanalyse"] == [] and off.last_reanalysis is None
    assert c_off["streams"] == [(500, 4), (504, 2), (506, 4), (510, 2)]
    assert "reanalyse_s" not in off.phase_times
    assert all(s.reanalysis is None for s in off.trainExamplesHistory)
    on, c_on = _learn(monkeypatch, tmp_path, "on", reanalyseFraction=0.5)
    n = 4 * 48
    # iteration 1 has no older iteration; iteration 2 reanalyses the first shard under (seed, key = 2, base 0)
    assert c_on["select"] == [(n, 21, 2, 0.5, 0)]
    assert len(c_on["reanalyse"]) == 1
    window, shard, idx, out, kw = c_on["reanalyse"][0]
    want = RR.select(n, 0, 21, 2, 0.5)
    m = len(want)
    assert window == 2 and np.array_equal(idx.cpu().numpy(), want) and 0 < m < n
    assert c_on["streams"] == [(500, 4), (504, 2), (506, 4), (510, m), (510 + m, 2)]
    assert kw["env_base"] == 510 and kw["sims"] == 4 and kw["seed"] == 21 and kw["cpuct"] == 1.5
    assert on.trainExamplesHistory[0] is out and on.trainExamplesHistory[1].reanalysis is None  # the newest: untouched
    assert on.last_reanalysis == [dict(item=0, n=n, reanalysed=m, n_empty=out.reanalysis["n_empty"])]
    # the first iteration's games do not depend on the knob: `shard` is the off run's first shard
    first = off.trainExamplesHistory[0]
    assert torch.equal(shard.states, first.states) and torch.equal(shard.policies["pi_vals"], first.policies["pi_vals"])
    # changed rows are among the chosen ones (a search may reproduce a row); the others are bit-identical
    ro, rs = _policy_rows(out, range(n)), _policy_rows(shard, range(n))
    changed = [i for i in range(n) if ro[i] != rs[i]]
    assert changed and set(changed) <= set(want.tolist())
    t_o, t_s = out.targets.cpu().numpy(), shard.targets.cpu().numpy()
    assert set(np.nonzero(t_o != t_s)[0].tolist()) <= set(want.tolist())
    assert out.values is shard.values and out.states is shard.states
    assert "reanalyse_s" in on.phase_times and on.phase_times["reanalyse_s"] > 0
    assert abs(sum(v for k, v in on.phase_times.items() if k != "iteration_s") - on.phase_times["iteration_s"]) < 1e-6
