"""Symmetry augmentation on the GPU (yk_examples_augment, K.augment_examples, NNetWrapper.train with
args.symmetries) against the restatement of tests/symmetry_ref.py, which
tests/test_symmetry_host.py holds to the oracle's game functions.

* the device equals the restatement bit for bit - boards, targets, policy rows in ascending order with their
  values - on hand-made states, a self-play shard with its real CSR and crafted rows;
* no flag copies; a row range with its index_base is that range of the whole call; `out` is reused;
* training with symmetries on is training on the restatement's augmented shard, bit for bit.
"""
import numpy as np
import pytest

import symmetry_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A = R.ASIZE
ALL = R.CARRY | R.ROLLS | R.GROUPS
N_GAMES, SIMS = 4, 8


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import kernels as K
    from yacht_amd import nnet
    from yacht_amd import replay
    return K, nnet, replay


@pytest.fixture(scope="module")
def shard(T):
    """The 192 pooled examples of a 4-game x 8-simulation hash-prior self-play, with their real CSR."""
    from yacht_amd.engine import SelfPlayEngine
    K, N, RP = T
    eng = SelfPlayEngine(N_GAMES, SIMS, 1.5, 15, prior="hash", max_moves=48)
    eng.run(23, 100)
    assert eng.stats()["errors"] == 0
    sh = RP.examples_from_images(eng.pack_records(), N_GAMES, 48, SIMS)
    eng.close()
    assert len(sh) == 192 and int(sh.policies["pi_indptr"][-1]) > 192
    return sh


@pytest.fixture(scope="module")
def rows(shard):
    """Host arrays of every row the bit-for-bit test runs, one CSR: the hand-made states with random
    in-range targets (and three random columns each), the shard, and crafted rows - empty, one entry, 65
    entries, all 3024 valid actions of a 10-dice node, 65 bids, and entries at undecodable actions."""
    rng = np.random.RandomState(3)
    H = R.hand_states()
    h = shard.host()
    states, targets, rws = [], [], []

    def add(s, t, cols):
        cols = np.unique(np.asarray(cols, dtype=np.int32))
        states.append(s)
        targets.append(t)
        rws.append((cols, rng.randint(1, 1000, len(cols)) / 1024.0))

    for s in H:
        add(s, rng.randint(0, A), rng.choice(A, 3, replace=False))
    for k in range(len(shard)):
        a0, a1 = h["pi_indptr"][k], h["pi_indptr"][k + 1]
        states.append(h["states"][k])
        targets.append(h["targets"][k])
        rws.append((h["pi_cols"][a0:a1].copy(), h["pi_vals"][a0:a1].copy()))
    ten, five, bid = H[6], H[8], H[2]
    from oracle import oracle as O
    valid10 = np.flatnonzero(O.valid(ten, 1)[0][0])
    assert len(valid10) == 3024 and (int(five[1]) >> 40) & 0xF == 5
    add(ten, 202 + 251, [])
    add(ten, 202 + 100, [202 + 252 * 11 + 251])
    add(ten, 3225, valid10[rng.permutation(3024)[:65]])
    add(ten, 202, valid10)
    add(bid, 201, rng.choice(202, 65, replace=False))
    add(five, 17, [17, 150, 202, 202 + 1, 202 + 252 * 2, 202 + 252 * 2 + 251, 3225])  # bids in the score phase,
    add(bid, 202 + 7, [0, 101, 202, 202 + 252 * 5 + 30, 3225])                        # combos past the carry
    add(ten, 0, np.arange(A))                                                         # every column there is
    lens = np.array([len(c) for c, _ in rws])
    assert {0, 1, 65, 3024, A} <= set(lens.tolist()) and lens.max() > 64
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(states=np.array(states, dtype=np.uint64), targets=np.array(targets, dtype=np.int32), indptr=indptr,
                cols=np.concatenate([c for c, _ in rws]).astype(np.int32),
                vals=np.concatenate([v for _, v in rws]).astype(np.float64), n_hand=len(H), n_shard=len(shard))


def _dev(T, rows):
    K = T[0]
    return (K.states_to_device(rows["states"]), torch.from_numpy(rows["targets"]).cuda(),
            tuple(torch.from_numpy(rows[k]).cuda() for k in ("indptr", "cols", "vals")))


_NAMES = {R.CARRY: ("carry",), R.ROLLS: ("rolls",), R.GROUPS: ("groups",), ALL: ("carry", "rolls", "groups")}


# ---------------------------------------------------------------- 1. device == restatement
@pytest.mark.parametrize("key", [0, 0xFFFFFFF1])
@pytest.mark.parametrize("seed", [6, 0xFEDCBA9876543210])
@pytest.mark.parametrize("flags", [R.CARRY, R.ROLLS, R.GROUPS, ALL])
def test_device_is_the_restatement_bit_for_bit(T, rows, flags, seed, key):
    K = T[0]
    S, tg, pol = _dev(T, rows)
    before = [x.clone() for x in (S, tg, *pol)]
    base = 1000
    s2, t2, p2 = K.augment_examples(S, tg, pol, seed, key, _NAMES[flags], index_base=base)
    es, et, ec, ev = R.augment(rows["states"], rows["targets"], rows["indptr"], rows["cols"], rows["vals"], seed, key,
                               flags, base)
    assert np.array_equal(K.states_to_host(s2), es)
    assert np.array_equal(t2.cpu().numpy(), et)
    c2, v2 = p2[1].cpu().numpy(), p2[2].cpu().numpy()
    assert c2.dtype == np.int32 and v2.dtype == np.float64
    assert np.array_equal(c2, ec) and v2.tobytes() == ev.tobytes()
    ip = rows["indptr"]
    for k in range(len(ip) - 1):
        assert (np.diff(c2[ip[k]:ip[k + 1]]) > 0).all(), k
    assert p2[0] is pol[0]  # indptr is shared, not copied
    for x, y in zip((S, tg, *pol), before):  # and no input was touched
        assert torch.equal(x, y)
    moved = int((es != rows["states"]).any(1).sum()), int((et != rows["targets"]).sum()), int((ec != rows["cols"]).sum())
    print(f"flags {flags}: {moved[0]} boards, {moved[1]} targets, {moved[2]} columns changed")
    assert moved[0] > 0 and all((m > 0) == (flags != R.ROLLS) for m in moved[1:])  # (rolls move no action)


def test_states_alone_and_targets_alone(T, rows):
    """targets and the CSR are optional, each on its own."""
    K = T[0]
    S, tg, pol = _dev(T, rows)
    es, et, ec, ev = R.augment(rows["states"], rows["targets"], rows["indptr"], rows["cols"], rows["vals"], 9, 4, ALL)
    s2, t2, p2 = K.augment_examples(S, None, None, 9, 4, ("carry", "rolls", "groups"))
    assert t2 is None and p2 is None and np.array_equal(K.states_to_host(s2), es)
    s2, t2, p2 = K.augment_examples(S, tg, None, 9, 4, ("carry", "rolls", "groups"))
    assert p2 is None and np.array_equal(K.states_to_host(s2), es) and np.array_equal(t2.cpu().numpy(), et)
    s2, t2, p2 = K.augment_examples(S, None, pol, 9, 4, ("carry", "rolls", "groups"))
    assert t2 is None and np.array_equal(p2[1].cpu().numpy(), ec) and p2[2].cpu().numpy().tobytes() == ev.tobytes()


# ---------------------------------------------------------------- 2. no flag: a copy
def test_no_symmetry_returns_the_inputs(T, rows):
    K = T[0]
    S, tg, pol = _dev(T, rows)
    s2, t2, p2 = K.augment_examples(S, tg, pol, 6, 5, ())
    assert torch.equal(s2, S) and torch.equal(t2, tg) and torch.equal(p2[1], pol[1]) and torch.equal(p2[2], pol[2])
    assert s2.data_ptr() != S.data_ptr() and p2[1].data_ptr() != pol[1].data_ptr()


# ---------------------------------------------------------------- 3. row ranges, out=
def test_a_row_range_is_that_range_of_the_whole_call(T, rows):
    K = T[0]
    S, tg, pol = _dev(T, rows)
    names = ("carry", "rolls", "groups")
    whole = K.augment_examples(S, tg, pol, 6, 5, names)
    n = S.shape[0]
    ip = rows["indptr"]
    for a, b in ((0, 1), (17, 83), (n - 9, n)):
        out_c, out_v = torch.full_like(pol[1], -7), torch.full_like(pol[2], -7.0)
        part = K.augment_examples(S[a:b], tg[a:b], (pol[0][a:b + 1], pol[1], pol[2]), 6, 5, names, index_base=a,
                                  out=(None, None, (None, out_c, out_v)))
        assert torch.equal(part[0], whole[0][a:b]) and torch.equal(part[1], whole[1][a:b])
        assert part[2][1] is out_c and part[2][2] is out_v
        assert torch.equal(out_c[ip[a]:ip[b]], whole[2][1][ip[a]:ip[b]])
        assert torch.equal(out_v[ip[a]:ip[b]], whole[2][2][ip[a]:ip[b]])
        # nothing outside the range's entries was written
        assert bool((out_c[:ip[a]] == -7).all()) and bool((out_c[ip[b]:] == -7).all())
        assert bool((out_v[:ip[a]] == -7).all()) and bool((out_v[ip[b]:] == -7).all())
    # out= : the same tensors come back, holding the new call's result
    again = K.augment_examples(S, tg, pol, 6, 8, names, out=whole)
    assert all(x is y for x, y in zip((again[0], again[1], again[2][1], again[2][2]),
                                      (whole[0], whole[1], whole[2][1], whole[2][2])))
    es, et, ec, ev = R.augment(rows["states"], rows["targets"], rows["indptr"], rows["cols"], rows["vals"], 6, 8, ALL)
    assert np.array_equal(K.states_to_host(again[0]), es) and np.array_equal(again[2][1].cpu().numpy(), ec)


def test_a_column_that_is_no_action_is_skipped_and_the_wrapper_refuses_it(T, rows):
    """Columns -1 and 3226 in one row: every other row is still the restatement's (nothing was written
    outside the bitmap or the row), and check_policy_columns raises."""
    K = T[0]
    S, tg, pol = _dev(T, rows)
    k = rows["n_hand"] + rows["n_shard"] + 2  # the 65-entry row
    ip = rows["indptr"]
    cols = pol[1].clone()
    cols[ip[k]] = -1
    cols[ip[k] + 1] = A
    with pytest.raises(ValueError, match="policy columns"):
        K.check_policy_columns((pol[0], cols, pol[2]))
    K.check_policy_columns(pol)
    s2, t2, p2 = K.augment_examples(S, tg, (pol[0], cols, pol[2]), 6, 5, ("carry", "rolls", "groups"))
    torch.cuda.synchronize()
    es, et, ec, ev = R.augment(rows["states"], rows["targets"], rows["indptr"], rows["cols"], rows["vals"], 6, 5, ALL)
    keep = np.ones(len(ec), dtype=bool)
    keep[ip[k]:ip[k + 1]] = False
    assert np.array_equal(p2[1].cpu().numpy()[keep], ec[keep]) and np.array_equal(p2[2].cpu().numpy()[keep], ev[keep])
    assert np.array_equal(K.states_to_host(s2), es) and np.array_equal(t2.cpu().numpy(), et)


# ---------------------------------------------------------------- 4. training
def _wrapper(N, sd, amp, target, symmetries=None):
    from yacht_amd.utils import dotdict
    args = dotdict(lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=32, vloss_weight=1.5, cuda=True, hidden=64,
                   nblocks=1, dropout=0.1, amp=amp, seed=6, policy_target=target)
    if symmetries is not None:
        args["symmetries"] = symmetries
    game = type("Game", (), {"getActionSize": lambda self: A})()
    w = N.NNetWrapper(game, args)
    w.nnet.load_state_dict(sd)
    return w


def _everything(w):
    tr = w._tr
    m, v = tr.moments()
    out = [tr.params().cpu().numpy().tobytes(), b"".join(m[k].numpy().tobytes() for k in m),
           b"".join(v[k].numpy().tobytes() for k in v), tr.step_count,
           b"".join(t.numpy().tobytes() for t in w.nnet.state_dict().values())]
    if tr.amp:
        out.append(sorted(tr.amp_state().items()))
    return out


@pytest.mark.parametrize("amp", [True, False])
@pytest.mark.parametrize("target", ["argmax", "visits"])
def test_training_with_symmetries_is_training_on_the_restatements_shard(T, shard, target, amp):
    """Model A: two one-epoch train calls with symmetries on.  Model B: symmetries off, fed the restatement's
    augmented shard for epoch keys 0 and its step count after the first call.  Bit-equal parameters,
    moments and AMP state - and not those of training on the plain shard."""
    K, N, RP = T
    torch.manual_seed(2)
    sd = {k: v.detach().clone() for k, v in N.YachtNNet(hidden=64, nblocks=1, dropout=0.0).state_dict().items()}
    h = shard.host()
    a = _wrapper(N, sd, amp, target, ("carry", "rolls", "groups"))
    a.train(shard, verbose=False)
    a.train(shard, verbose=False)

    b = _wrapper(N, sd, amp, target)
    keys = []
    for call in range(2):
        key = b._trainer().step_count
        keys.append(key)
        es, et, ec, ev = R.augment(h["states"], h["targets"], h["pi_indptr"], h["pi_cols"], h["pi_vals"], 6, key, ALL)
        pol = dict(pi_indptr=shard.policies["pi_indptr"], pi_cols=torch.from_numpy(ec).cuda(),
                   pi_vals=torch.from_numpy(ev).cuda(), values64=shard.policies["values64"])
        b.train(RP.ExampleShard(K.states_to_device(es), torch.from_numpy(et).cuda(), shard.values, policies=pol),
                verbose=False)
    assert keys[0] == 0 and 0 < keys[1] <= 6
    assert _everything(a) == _everything(b)

    c = _wrapper(N, sd, amp, target)
    c.train(shard, verbose=False)
    c.train(shard, verbose=False)
    assert _everything(c)[0] != _everything(a)[0]
    # and an empty symmetries tuple is the plain loop
    d = _wrapper(N, sd, amp, target, ())
    d.train(shard, verbose=False)
    d.train(shard, verbose=False)
    assert _everything(d) == _everything(c)
