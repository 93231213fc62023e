"""Config 5 on the GPU: the device replay buffer and the multi-rank Coach iteration
(Coach.py:74-139).

* yk_examples_from_records (the device replay buffer) against two independent host
  restatements: helpers.host_examples (numpy over the packed image) and coach.examples_from_records
  (the reference's per-move (board, pi, v) tuples, argmax'd as NNet.py:145-146 does);
* sharding: the images of games split over "ranks" pool into exactly the single-batch examples;
* two ranks (gloo) sharing GPU 0 run the Coach's pieces and Coach.learn: the pooled buffer is
  the union of both ranks' records and equals one process playing every game; both ranks hold
  bit-identical parameters after training, equal to the single-process train within f32
  summation order; the sharded gating arena's tally equals the single-GPU arena.
"""
import os
import socket

import numpy as np
import pytest

from helpers import host_examples
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ARGS = dict(numIters=1, numEps=6, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000, numMCTSSims=4,
            arenaCompare=6, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=2,
            batch_size=40, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3,
            amp=False)  # the float32 step: the DDP-split comparison below is held to f32 summation order


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import coach, engine, nnet, replay
    return coach, engine, nnet, replay


def _selfplay(E, net, n, sims, seed, base, max_moves=48):
    eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net, max_moves=max_moves)
    eng.run(seed, base)
    assert eng.stats()["errors"] == 0
    rec = eng.records()
    img = eng.pack_records()
    eng.close()
    return rec, img


def _assert_same_examples(shard, h, states_key="states"):
    assert len(shard) == len(h["targets"])
    assert np.array_equal(shard.states.cpu().numpy().view(np.uint64), h[states_key])
    assert np.array_equal(shard.targets.cpu().numpy(), h["targets"])
    assert np.array_equal(shard.values.cpu().numpy(), h["values"].astype(np.float32))


def test_examples_kernel_matches_host_restatements(Y):
    C, E, N, R = Y
    n, sims, seed, base = 96, 12, 41, 300
    net = N.YkNet(spec.closed_form_weights(256, 6), 256, 6)
    rec, img = _selfplay(E, net, n, sims, seed, base)
    shard = R.examples_from_images(img, n, 48, sims)
    h = host_examples(img.cpu().numpy(), n, 48, sims)
    _assert_same_examples(shard, h)
    # the reference's tuples (Coach.py:72) -> argmax(pi) (NNet.py:145-146), values, boards
    ref = [ex for ep in C.examples_from_records(rec, n) for ex in ep]
    assert len(ref) == len(shard) == n * 48
    from yacht_amd.state import pack_many
    assert np.array_equal(pack_many([b for b, _, _ in ref]), h["states"])
    assert np.array_equal(np.array([int(np.argmax(np.asarray(p))) for _, p, _ in ref], dtype=np.int32), h["targets"])
    assert np.array_equal(np.array([v for _, _, v in ref]), h["values"])
    # both temperatures occur, and a temp-1 target is not always the played action
    temp = rec["info"][:, :48, 0].reshape(-1)
    act = rec["info"][:, :48, 2].reshape(-1)
    assert (temp == 1).any() and (temp == 0).any() and (h["targets"][temp == 1] != act[temp == 1]).any()
    # the sparse policies are the reference's pi exactly
    for k in (0, 1, 13, 14, 15, 47, 48 * 5 + 3, len(ref) - 1):
        pi = np.zeros(3226)
        a0, a1 = h["pi_indptr"][k], h["pi_indptr"][k + 1]
        pi[h["pi_cols"][a0:a1]] = h["pi_vals"][a0:a1]
        assert np.array_equal(pi, np.asarray(ref[k][1], dtype=np.float64)), k
    # the deque's maxlen keeps the last examples; n_games trims whole games from the end
    tail = R.examples_from_images(img, n, 48, sims, maxlen=1000)
    assert len(tail) == 1000
    assert torch.equal(tail.targets, shard.targets[-1000:]) and torch.equal(tail.states, shard.states[-1000:])
    part = R.examples_from_images(img, n, 48, sims, n_games=7)
    assert len(part) == 7 * 48 and torch.equal(part.targets, shard.targets[:7 * 48])
    # the device policy CSR (yk_examples_policies) is the host restatement's, bit for bit, for the
    # whole batch and for a maxlen tail
    def _same_csr(got, want, skip=0):
        n = len(got["targets"])
        ip = want["pi_indptr"]
        a0, a1 = int(ip[skip]), int(ip[skip + n])
        assert np.array_equal(got["pi_indptr"], ip[skip:skip + n + 1] - a0)
        assert np.array_equal(got["pi_cols"], want["pi_cols"][a0:a1])
        assert np.array_equal(got["pi_vals"], want["pi_vals"][a0:a1])
        assert np.array_equal(got["values"], want["values"][skip:skip + n])
        assert np.array_equal(got["states"], want["states"][skip:skip + n])
    _same_csr(shard.host(), h)
    _same_csr(tail.host(), h, skip=len(ref) - 1000)
    _same_csr(part.host(), h)
    # (the whole batch's CSR is 4608 rows: every thread of the one-workgroup scan owns 5 of them.)  The image
    # 11 times over is 1056 games - the example offsets' scan then owns two games per thread - and gives the
    # single image's examples 11 times over
    many = R.examples_from_images(torch.stack([img] * 11), n, 48, sims).host()
    one = shard.host()
    for k in ("states", "targets", "values", "pi_cols", "pi_vals"):
        assert np.array_equal(many[k], np.concatenate([one[k]] * 11)), k
    nnz = int(one["pi_indptr"][-1])
    assert np.array_equal(many["pi_indptr"],
                          np.concatenate([[0]] + [one["pi_indptr"][1:] + r * nnz for r in range(11)]))
    # lazy reference tuples of a shard
    b, pi, v = tail[0]
    assert pi == ref[len(ref) - 1000][1] and v == ref[len(ref) - 1000][2]
    assert [int(x) for x in pack_many([b])[0]] == [int(x) for x in h["states"][len(ref) - 1000]]


def test_sharded_images_pool_into_the_single_batch(Y):
    """What the all-gather builds: images of games [0, c) and [c, 2c) (two ranks, stream
    env0 + k for game k) give exactly the examples of one engine playing all games; a short
    last shard is trimmed with n_games."""
    C, E, N, R = Y
    n, sims, seed, base = 45, 6, 77, 1000
    net = N.YkNet(spec.closed_form_weights(256, 6), 256, 6)
    _, whole = _selfplay(E, net, n, sims, seed, base)
    c = 23
    imgs = [_selfplay(E, net, c, sims, seed, base + r * c)[1] for r in range(2)]
    pooled = R.examples_from_images(torch.stack(imgs), c, 48, sims, n_games=n)
    single = R.examples_from_images(whole, n, 48, sims)
    assert len(pooled) == len(single) == n * 48
    for k in ("states", "targets", "values"):
        assert torch.equal(getattr(pooled, k), getattr(single, k)), k


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _coach_worker(rank, world, port, ckdir, out):
    import sys
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (here, os.path.join(here, "nypc-yacht-auction_amd")):
        sys.path.insert(0, p)
    torch.cuda.set_device(0)  # both ranks share the one GPU of the box
    from yacht_amd.arena import GatingArena
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    args = dotdict(ARGS, checkpoint=ckdir, load_folder_file=(ckdir, "best.pth.tar"))
    torch.manual_seed(5)
    game = YachtGame(seed=21, env_id=500)
    coach = Coach(game, NNetWrapper(game, args), args)
    # the pieces: sharded self-play + all-gather, DDP train, sharded gating arena
    shard = coach.selfPlayExamples(args.numEps)
    out[f"ex{rank}"] = (shard.states.cpu().numpy(), shard.targets.cpu().numpy(), shard.values.cpu().numpy())
    coach.pnet.nnet.load_state_dict(coach.nnet.nnet.state_dict())
    coach.nnet.train([shard], verbose=False)
    out[f"p{rank}"] = {k: v.numpy().copy() for k, v in coach.nnet.nnet.state_dict().items()}
    out[f"pit{rank}"] = GatingArena(game, coach.pnet, coach.nnet, args).playGames(args.arenaCompare, env_base=900)
    # DDP split: the minibatch split over the ranks, gradients all-reduced
    ws = NNetWrapper(game, dotdict(args, ddp_batch="split"))
    ws.nnet.load_state_dict(coach.pnet.nnet.state_dict())
    ws.train([shard], verbose=False)
    out[f"ps{rank}"] = {k: v.numpy().copy() for k, v in ws.nnet.state_dict().items()}
    # the same split in the default mode under args.cuda (autocast + GradScaler): row-offset
    # backward, the all-reduce, the unfused apply with the GradScaler state
    wa = NNetWrapper(game, dotdict(args, ddp_batch="split", amp=True))
    wa.nnet.load_state_dict(coach.pnet.nnet.state_dict())
    wa.train([shard], verbose=False)
    out[f"pa{rank}"] = ({k: v.numpy().copy() for k, v in wa.nnet.state_dict().items()}, wa._trainer().amp_state())
    # DDP weak scaling: every rank its own batch_size rows (a global minibatch of 2 x batch_size)
    wk = NNetWrapper(game, dotdict(args, ddp_batch="per_rank"))
    wk.nnet.load_state_dict(coach.pnet.nnet.state_dict())
    wk.train([shard], verbose=False)
    out[f"pr{rank}"] = ({k: v.numpy().copy() for k, v in wk.nnet.state_dict().items()}, wk._trainer().step_count)
    # the loop itself (files written by rank 0, read back by every rank)
    coach.learn()
    out[f"learn{rank}"] = (coach.last_pit, len(coach.trainExamplesHistory[-1]),
                           {k: v.numpy().copy() for k, v in coach.nnet.nnet.state_dict().items()})
    dist.destroy_process_group()


def _train_split_emulated(wrapper, examples, world):
    """NNetWrapper.train's ddp_batch "split" (nnet.py) in one process: per minibatch, each rank's
    share through backward at its row offset, scaled by its share (dist.allreduce_grads' mul_ on
    the device), the shares summed in f32 on the host as the gloo all-reduce sums them, apply."""
    from yacht_amd.replay import as_device_examples
    tr = wrapper._trainer()
    states, targets, values = as_device_examples(examples)
    n, bs = states.shape[0], wrapper.args.batch_size
    g = torch.Generator(device="cuda")
    g.manual_seed(int(wrapper.args.get("seed", 0)) + 1000003 * tr.step_count)
    for _ in range(wrapper.args.epochs):
        perm = torch.randperm(n, generator=g, device="cuda").to(torch.int32)
        for i in range(0, n, bs):
            idx = perm[i:i + bs]
            parts = torch.tensor_split(idx, world)
            total = None
            for r, loc in enumerate(parts):
                b = loc.numel()
                if b:
                    tr.backward(states, targets, values, idx=loc, row0=sum(int(x.numel()) for x in parts[:r]))
                    gr = tr.grads().clone()
                else:
                    gr = torch.zeros_like(tr.grads())
                gr.mul_(float(b / idx.numel()))
                total = gr.cpu() if total is None else total + gr.cpu()
            tr.grads().copy_(total.to("cuda"))
            tr.apply()
    with torch.no_grad():
        wrapper.nnet.load_state_dict(tr.state_dict())
    wrapper._yk = None


def test_coach_iteration_two_ranks_sharing_gpu0(Y, tmp_path):
    import torch.multiprocessing as mp
    C, E, N, R = Y
    from yacht_amd.arena import GatingArena
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    ck = str(tmp_path / "ck")
    mp.start_processes(_coach_worker, args=(2, _free_port(), ck, out), nprocs=2, start_method="spawn")
    # the pooled buffer: identical on both ranks, the union of the ranks' games in env-id order
    # (rank 0 played envs 500-502, rank 1 503-505), equal to one process playing all six
    for a, b in zip(out["ex0"], out["ex1"]):
        assert np.array_equal(a, b)
    args = dotdict(ARGS, checkpoint=str(tmp_path / "single"), load_folder_file=(str(tmp_path), "x"))
    torch.manual_seed(5)
    game = YachtGame(seed=21, env_id=500)
    coach = C.Coach(game, NNetWrapper(game, args), args)
    single = coach.selfPlayExamples(args.numEps)
    assert len(single) == 6 * 48
    assert np.array_equal(single.states.cpu().numpy(), out["ex0"][0])
    assert np.array_equal(single.targets.cpu().numpy(), out["ex0"][1])
    assert np.array_equal(single.values.cpu().numpy(), out["ex0"][2])
    net0 = NNetWrapper(game, args)
    net0.nnet.load_state_dict(coach.nnet.nnet.state_dict())
    _, img1 = _selfplay(E, coach.nnet.yk_net(), 3, 4, 21, 503)  # rank 1's own games
    part = R.examples_from_images(img1, 3, 48, 4)
    assert torch.equal(part.targets.cpu(), torch.from_numpy(out["ex0"][1][3 * 48:]))
    # replicated (the default): every rank takes the whole minibatch's step - bit-identical to the
    # single-process train, no collective
    p0, p1 = out["p0"], out["p1"]
    assert all(np.array_equal(p0[k], p1[k]) for k in p0)
    coach.nnet.train([single], verbose=False)
    sp = coach.nnet.nnet.state_dict()
    assert all(np.array_equal(p0[k], sp[k].numpy()) for k in p0)
    # DDP split: both ranks bit-identical; equal to the single-process train up to f32 summation order
    ps0, ps1 = out["ps0"], out["ps1"]
    assert all(np.array_equal(ps0[k], ps1[k]) for k in ps0)
    a = np.concatenate([ps0[k].reshape(-1) for k in ps0]).astype(np.float64)
    b = np.concatenate([sp[k].numpy().reshape(-1) for k in ps0]).astype(np.float64)
    # AdamW divides by sqrt(v) + eps, so a gradient entry near eps can move its weight by up to
    # 2 lr on a summation-order change; everything else agrees to f32 rounding
    assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-4
    assert (np.abs(a - b) > 1e-5).mean() < 1e-3
    # AMP split: both ranks bit-identical with the same GradScaler state, and equal bit for bit to
    # one process that forms the same two half-batch gradients (each rank's fp16 backward at its
    # row offset, x its share), sums them in f32 as the all-reduce does and applies - so every
    # GradScaler skip decision coincides (the unsplit AMP train can skip a different step)
    pa0, pa1 = out["pa0"], out["pa1"]
    assert all(np.array_equal(pa0[0][k], pa1[0][k]) for k in pa0[0]) and pa0[1] == pa1[1]
    wam = NNetWrapper(game, dotdict(args, amp=True))
    wam.nnet.load_state_dict(net0.nnet.state_dict())
    _train_split_emulated(wam, [single], world=2)
    st1 = wam._trainer().amp_state()
    assert wam._trainer().amp and st1 == pa0[1] and st1["steps"] > 0
    assert all(np.array_equal(pa0[0][k], wam.nnet.state_dict()[k].numpy()) for k in pa0[0])
    # per_rank: the single-process train at batch 2 x batch_size, in half the steps
    pr0, pr1 = out["pr0"], out["pr1"]
    assert all(np.array_equal(pr0[0][k], pr1[0][k]) for k in pr0[0])
    wide = NNetWrapper(game, dotdict(args, batch_size=2 * args.batch_size))
    wide.nnet.load_state_dict(net0.nnet.state_dict())
    wide.train([single], verbose=False)
    assert pr0[1] == wide._trainer().step_count == 2 * -(-len(single) // (2 * args.batch_size))
    a = np.concatenate([pr0[0][k].reshape(-1) for k in pr0[0]]).astype(np.float64)
    b = np.concatenate([wide.nnet.state_dict()[k].numpy().reshape(-1) for k in pr0[0]]).astype(np.float64)
    assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-4 and (np.abs(a - b) > 1e-5).mean() < 1e-3
    # the sharded gating arena's tally is the single-GPU arena's on the same two nets: the
    # ranks' previous net (the initial weights, net0) against their trained p0
    newnet = NNetWrapper(game, args)
    newnet.nnet.load_state_dict({k: torch.from_numpy(v) for k, v in p0.items()})
    pit = GatingArena(game, net0, newnet, args).playGames(args.arenaCompare, env_base=900)
    assert out["pit0"] == out["pit1"]
    assert sum(out["pit0"]) == 6
    assert tuple(pit) == tuple(out["pit0"])
    # Coach.learn on two ranks: same verdict, examples and parameters on both
    l0, l1 = out["learn0"], out["learn1"]
    assert l0[0] == l1[0] and l0[1] == l1[1] == 6 * 48
    assert all(np.array_equal(l0[2][k], l1[2][k]) for k in l0[2])
    for f in ("temp.pth.tar", "checkpoint_0.pth.tar.examples.npz"):
        assert os.path.exists(os.path.join(ck, f)), f
