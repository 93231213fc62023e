"""The playout cap randomization restated (include/yacht_hip.h, yk_engine_set_playout_cap /
yk_playout_schedule / yk_examples_full_rows / yk_policies_take): the schedule from oracle/spec.py's Philox, a
capped episode as a step-by-step Coach.executeEpisode loop over the plugin classes - each move one
MCTS.search_counts(canon, sims = the move's cap), the per-call `sims` the plugin has always taken - and numpy
versions of the full-row selection and the CSR take."""
import numpy as np

from oracle import spec

A = 3226
DOMAIN = 0x30000000  # counter word 3 of the schedule draws
REC_FAST = 0x100     # info[..., 6] of a fast move
M32, M64 = 0xFFFFFFFF, 2**64 - 1


def uniform(seed, env_base, move, domain=DOMAIN):
    """u of move `move` of the batch (seed, env_base): counter (move, env_base, 0, domain), key (seed lo, seed hi),
    x = x0 | x1 << 32, u = (x >> 11) * 2^-53."""
    seed = int(seed) & M64
    x0, x1, _, _ = spec.philox4x32_10(int(move) & M32, int(env_base) & M32, 0, domain, seed & M32, seed >> 32)
    return float((x0 | (x1 << 32)) >> 11) * (1.0 / 9007199254740992.0)


def schedule(seed, env_base, full_prob, n_moves):
    """bool[n_moves]: move m is a full move iff its uniform lies below full_prob."""
    return np.asarray([uniform(seed, env_base, m) < full_prob for m in range(int(n_moves))], dtype=bool)


def show(full):
    return "".join("F" if f else "." for f in full)


def episode(game, mcts, caps, temp_threshold):
    """Coach.executeEpisode (Coach.py:34-72) step by step over the plugin classes, move m searched with caps[m]
    simulations: what a one-game engine batch records.  game: a fresh yacht_amd.game.YachtGame; mcts: an MCTS
    over it.  Returns dict(actions, ctr[M][2], counts[M][3226], canon[M][8], players, values, final[8],
    n_moves)."""
    from yacht_amd.state import pack
    board, cur, step = game.getInitBoard(), 1, 0
    actions, ctr, counts, canon_w, players = [], [], [], [], []
    while True:
        m = step
        step += 1
        canon = game.getCanonicalForm(board, cur)
        c0 = game.rng.ctr
        cnt = mcts.search_counts(canon, sims=int(caps[m]))
        if step < temp_threshold:  # temp 1: np.random.choice(len(pi), p=counts / sum)  (Coach.py:58-65)
            p = np.asarray(cnt, dtype=np.float64)
            p = p / float(sum(float(x) for x in cnt))
            cdf = p.cumsum()
            cdf /= cdf[-1]
            action = int(cdf.searchsorted(game.rng.uniform53(), side="right"))
        else:  # temp 0: np.random.choice(bestAs) (MCTS.py:44-49), then Coach's draw over the one-hot pi
            mx = max(cnt)
            best = [a for a, c in enumerate(cnt) if c == mx]
            action = best[game.rng.below(len(best))]
            game.rng.uniform53()
        actions.append(action)
        ctr.append((c0, game.rng.ctr))
        counts.append(np.asarray(cnt, dtype=np.int32))
        canon_w.append(np.asarray(pack(canon), dtype=np.uint64))
        players.append(cur)
        board, cur = game.getNextState(board, cur, action)
        r = game.getGameEnded(board, cur)
        if r != 0:
            break
    values = [r * (1.0 if p == cur else -1.0) for p in players]
    return dict(actions=np.asarray(actions, dtype=np.int32), ctr=np.asarray(ctr, dtype=np.uint64),
                counts=np.asarray(counts), canon=np.asarray(canon_w), players=np.asarray(players, dtype=np.int32),
                values=np.asarray(values, dtype=np.float64), final=np.asarray(pack(board), dtype=np.uint64),
                n_moves=len(actions))


def full_rows(infos, n_moves, n_games=-1):
    """The example numbers (int32, ascending) of the full moves.  infos: a list of info arrays [E][M][8], one per
    image; n_moves: the matching list of [E] arrays; the examples are numbered in (image, game, move) order over
    the first n_games games (< 0 or more than there are: all).  Returns (idx, total)."""
    idx, k, g = [], 0, 0
    all_games = sum(len(nm) for nm in n_moves)
    n_games = all_games if n_games < 0 or n_games > all_games else n_games
    for info, nm in zip(infos, n_moves):
        M = info.shape[1]
        for e in range(len(nm)):
            if g >= n_games:
                break
            g += 1
            for m in range(min(max(int(nm[e]), 0), M)):
                if not int(info[e, m, 6]) & REC_FAST:
                    idx.append(k)
                k += 1
    return np.asarray(idx, dtype=np.int32), k


def take(indptr, cols, vals, idx):
    """Rows idx (any order, repeats allowed) of the CSR as a new CSR (indptr int64, cols int32, vals float64)."""
    n = len(indptr) - 1
    out_ip, out_c, out_v = [0], [], []
    for r in (int(x) for x in idx):
        assert 0 <= r < n
        a, b = int(indptr[r]), int(indptr[r + 1])
        out_c.append(np.asarray(cols[a:b], dtype=np.int32))
        out_v.append(np.asarray(vals[a:b], dtype=np.float64))
        out_ip.append(out_ip[-1] + (b - a))
    return (np.asarray(out_ip, dtype=np.int64), np.concatenate(out_c) if out_c else np.zeros(0, dtype=np.int32),
            np.concatenate(out_v) if out_v else np.zeros(0, dtype=np.float64))
