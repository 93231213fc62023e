"""First-play urgency restated (include/yacht_hip.h, yk_engine_set_fpu / yk_fpu_pick).
TEST INFRASTRUCTURE ONLY.

The rule in plain Python ints and floats (P is the float32 the search holds; numpy.float32 only for the last two
steps), at a node with Ns > 0, a visited and an unvisited valid edge:
  visited candidate     the largest u = Q + cpuct P sqrt(Ns) / (1 + N) as the reference computes it (float32; +inf
                        for a forced edge), the lowest action among equals
  unvisited candidate   the largest x = (f32(cpuct) P) f32(sqrt(Ns + 1e-8)), the lowest action among equals
  parent estimate       W  = sum N * int(round(Q * 2**32)), Mi = sum int(float(P) * 2**40) over the visited edges
                        fq = float32((W / Ns) / 2**32 - r * sqrt(Mi / 2**40))
  winner                float32(fq) + float32(x) against u: the larger, the lower action on equality
on top of forced_ref's Coach / MCTS (noise_ref's with the forced test): FpuMCTS applies the rule at every depth -
r_root at depth 0 - and counts what it did; play_episode is forced_ref's with the rule in every search of the
game (fast moves of the playout cap too); arena_game is Arena.playGame over the same searches."""
import math

import numpy as np

import forced_ref as F
import noise_ref as R
from oracle import oracle as O
from oracle import spec

ASIZE = R.ASIZE
REC_FAST = F.REC_FAST
TWO32, TWO40 = 2 ** 32, 2 ** 40


# ------------------------------------------------------------------ the rule (normative)
def w_term(N, Q):
    return int(N) * int(round(float(Q) * TWO32))  # (round: ties to even)


def m_term(P):
    return int(float(P) * TWO40)  # (truncated)


def fpu_value(W, Mi, Ns, r):
    """fq from the two integer sums: every order of summation gives the same W and Mi."""
    qbar = (float(W) / float(Ns)) / float(TWO32)
    mass = float(Mi) / float(TWO40)
    return np.float32(qbar - float(r) * math.sqrt(mass))


def unvisited_wins(fq, x, ju, u, jv):
    uu = np.float32(fq) + np.float32(x)
    return bool(uu > u or (uu == u and ju < jv))


def pick(u_vis, x_unv, terms, Ns, r):
    """One node: u_vis {index: u of a visited edge}, x_unv {index: x of an unvisited edge}, terms [(N, Q, P)] of
    the visited edges -> (index, unvisited won, the rule decided).  A node at Ns = 0 or with one kind of edge:
    the plain argmax over both, the lowest index among equals."""
    jv = min(u_vis, key=lambda j: (-u_vis[j], j)) if u_vis else None
    ju = min(x_unv, key=lambda j: (-x_unv[j], j)) if x_unv else None
    if jv is None and ju is None:
        return -1, False, False
    if jv is not None and ju is not None and Ns > 0:
        fq = fpu_value(sum(w_term(N, Q) for N, Q, _ in terms), sum(m_term(P) for _, _, P in terms), Ns, r)
        won = unvisited_wins(fq, x_unv[ju], ju, u_vis[jv], jv)
        return (ju if won else jv), won, True
    if jv is None or (ju is not None and (x_unv[ju] > u_vis[jv] or (x_unv[ju] == u_vis[jv] and ju < jv))):
        return ju, True, False
    return jv, False, False


def fpu_pick(indptr, p, counts, q, ns, cpuct, r):
    """yk_fpu_pick in numpy: rows of a CSR -> (pick int32[n], unvisited int32[n])."""
    c32 = np.float32(cpuct)
    out, unv = [], []
    for row in range(len(indptr) - 1):
        a, b = int(indptr[row]), int(indptr[row + 1])
        Ns = max(int(ns[row]), 0)
        sq, sqe = np.float32(math.sqrt(Ns)), np.float32(math.sqrt(Ns + 1e-8))
        u_vis, x_unv, terms = {}, {}, []
        for i in range(a, b):
            cp = c32 * np.float32(p[i])
            if counts[i] > 0:
                u_vis[i - a] = np.float32(q[i]) + (cp * sq) / np.float32(int(counts[i]) + 1)
                terms.append((int(counts[i]), float(q[i]), p[i]))
            else:
                x_unv[i - a] = cp * sqe
        j, won, _ = pick(u_vis, x_unv, terms, Ns, r)
        out.append(j)
        unv.append(int(won))
    return np.array(out, dtype=np.int32), np.array(unv, dtype=np.int32)


# ------------------------------------------------------------------ Coach / MCTS in plain Python
class FpuMCTS(F.ForcedMCTS):
    """forced_ref.ForcedMCTS whose search applies the rule while `self.r` is not None: r at interior nodes,
    r_root at depth 0.  Counts, overall and per depth class (0 root, 1 interior): the picks the rule decided
    (`vis_wins` + `unv_wins`), who won, and how often the pick is not the reference rule's (`differs`)."""

    def __init__(self, seed, env, stream, sims, cpuct, r=None, r_root=None):
        super().__init__(seed, env, stream, sims, cpuct)
        self.r = r
        self.r_root = r if r_root is None else r_root
        self.vis_wins, self.unv_wins, self.differs = [0, 0], [0, 0], [0, 0]

    def leaf_value(self, board, v):
        """The value an expansion returns (negated): the prior's own.  tools/fpu_spread.py puts a stand-in here."""
        return v

    @property
    def fpu_picks(self):
        return sum(self.vis_wins) + sum(self.unv_wins)

    @property
    def fpu_unvisited_picks(self):
        return sum(self.unv_wins)

    def search(self, board, depth=0):  # forced_ref.ForcedMCTS.search with the rule
        s = board.tobytes()
        if s not in self.Es:
            self.Es[s] = float(O.ended(board, 1)[0][0])
        if self.Es[s] != 0:
            return -self.Es[s]
        if s not in self.Ps:
            pi, v = O.hash_prior(board)
            valids = O.valid(board, 1)[0][0].astype(np.float32)
            P = pi[0] * valids
            sum_Ps_s = np.sum(P)
            if sum_Ps_s > 0:
                P /= sum_Ps_s
            else:
                P = P + valids
                if np.sum(P) > 0:
                    P /= np.sum(P)
                else:
                    P = np.zeros(ASIZE, dtype=np.float32)
                    P[0] = 1.0
            self.Ps[s], self.Vs[s], self.Ns[s] = P, valids, 0
            self.expansions += 1
            return -self.leaf_value(board, v[0])
        valids = self.Vs[s]
        P = self.Ps[s]
        Ns = self.Ns[s]
        u = (np.float32(self.cpuct) * P) * np.float32(math.sqrt(Ns + R.EPS))
        u = np.where(valids > 0, u, -np.inf).astype(np.float64)
        visited = []
        for a in np.flatnonzero(valids):
            a = int(a)
            if (s, a) in self.Qsa:
                visited.append(a)
                u[a] = self.Qsa[(s, a)] + self.cpuct * P[a] * math.sqrt(Ns) / (1 + self.Nsa[(s, a)])
                if depth == 0 and self.k > 0 and F.forced(self.Nsa[(s, a)], P[a], Ns, self.k):
                    u[a] = np.inf
        a = int(np.argmax(u)) if u.size and np.max(u) > -np.inf else -1
        nvalid = int(np.count_nonzero(valids))
        if self.r is not None and Ns > 0 and visited and len(visited) < nvalid:
            vis = np.zeros(ASIZE, dtype=bool)
            vis[visited] = True
            uv = np.where(vis, u, -np.inf)
            ux = np.where((valids > 0) & ~vis, u, -np.inf)
            jv, ju = int(np.argmax(uv)), int(np.argmax(ux))  # (argmax: the first of the largest)
            W = sum(w_term(self.Nsa[(s, b)], self.Qsa[(s, b)]) for b in visited)
            Mi = sum(m_term(P[b]) for b in visited)
            fq = fpu_value(W, Mi, Ns, self.r_root if depth == 0 else self.r)
            # (u holds float32 values, or +inf for a forced edge: the conversions are exact)
            won = unvisited_wins(fq, np.float32(ux[ju]), ju, np.float32(uv[jv]), jv)
            cls = 0 if depth == 0 else 1
            (self.unv_wins if won else self.vis_wins)[cls] += 1
            new = ju if won else jv
            self.differs[cls] += new != a
            a = new
        if a == -1 or not valids[a]:
            va = np.flatnonzero(valids == 1)
            if len(va) == 0:
                return 0
            a = int(va[0])
        elif depth == 0 and u[a] == np.inf:
            self.forced_picks += 1
        nxt, npl, st, ctr = O.step(board, 1, a, self.seed, self.env, self.rs.ctr)
        assert st[0] == 0
        self.rs.ctr = int(ctr[0])
        v = self.search(O.canonical(nxt, npl)[0], depth + 1)
        if (s, a) in self.Qsa:
            self.Qsa[(s, a)] = (self.Nsa[(s, a)] * self.Qsa[(s, a)] + v) / (self.Nsa[(s, a)] + 1)
            self.Nsa[(s, a)] += 1
        else:
            self.Qsa[(s, a)] = v
            self.Nsa[(s, a)] = 1
        self.Ns[s] += 1
        return -v


def play_episode(seed, env, sims, r=None, r_root=None, k=0.0, prune=True, cpuct=1.5, temp_threshold=15, max_moves=48,
                 root_prior=None, full=None, fast_sims=0, mcts_class=None):
    """forced_ref.play_episode with first-play urgency (r, r_root; None: off) in every search of the game - the
    fast moves of the playout cap too, which are still neither noised, forced nor pruned.  Returns the record
    fields plus forced_picks, pruned_visits, raw, kept, and the rule's counts: fpu_picks, fpu_unvisited_picks,
    vis_wins / unv_wins / differs ([root, interior])."""
    board, ctr = O.init_board(seed, [env])
    board, rs = board[0], spec.Stream(seed, env, int(ctr[0]))
    mcts = (mcts_class or FpuMCTS)(seed, env, rs, sims, cpuct, r, r_root)
    cur, step = 1, 0
    states, info, ctrs, visits, voff, raws, kept = [], [], [], [], [0], [], []
    pruned_visits = 0
    while True:
        step += 1
        move = step - 1
        is_full = full is None or bool(full[move])
        canon = O.canonical(board, cur)[0]
        temp = int(step < temp_threshold)
        c0 = rs.ctr
        mcts.sims = sims if is_full else fast_sims
        mcts.k = float(k) if is_full else 0.0
        counts = mcts.get_action_counts(
            canon, None if root_prior is None or not is_full else (lambda P: root_prior(move, P)))
        s = canon.tobytes()
        root_ns = mcts.Ns.get(s, -1)
        acts = sorted(counts)
        n = [counts[a] for a in acts]
        raws.append(dict(counts))
        if is_full and k > 0 and prune and acts:
            got = F.prune_row(acts, n, [mcts.Qsa[(s, a)] for a in acts], [mcts.Ps[s][a] for a in acts], root_ns, k, cpuct)
            pruned_visits += sum(n) - sum(got)
            acts, n = [a for a, c in zip(acts, got) if c > 0], [c for c in got if c > 0]
        kept.append(dict(zip(acts, n)))
        if temp == 0:
            mx = max(n) if n else 0
            if mx == 0:
                action = rs.below(ASIZE)
            else:
                best = [a for a, c in zip(acts, n) if c == mx]
                action = best[rs.below(len(best))]
            rs.uniform53()
        else:
            total = float(sum(n))
            cdf, c = [], 0.0
            for x in n:
                c += x / total
                cdf.append(c)
            u = rs.uniform53()
            action = next(a for a, c in zip(acts, cdf) if c / cdf[-1] > u)
        states.append(canon)
        info.append([temp, cur, action, mcts.expansions, root_ns, len(acts), 0 if is_full else REC_FAST, 0])
        ctrs.append([c0, rs.ctr])
        visits += [[a, c] for a, c in zip(acts, n)]
        voff.append(len(visits))
        nxt, npl, st, ctr = O.step(board, cur, action, seed, env, rs.ctr)
        assert st[0] == 0
        rs.ctr = int(ctr[0])
        board, player, cur = nxt[0], cur, int(npl[0])
        info[-1][1] = player
        res = float(O.ended(board, cur)[0][0])
        if res != 0 or step >= max_moves:
            break
    players = np.array([i[1] for i in info])
    return dict(states=np.array(states, dtype=np.uint64), info=np.array(info, dtype=np.int32),
                ctr=np.array(ctrs, dtype=np.uint64), values=res * np.where(players != cur, -1.0, 1.0),
                final=board.astype(np.uint64), n_moves=step, visits=np.array(visits, dtype=np.int32).reshape(-1, 2),
                visits_off=np.array(voff, dtype=np.int64), forced_picks=mcts.forced_picks,
                pruned_visits=pruned_visits, raw=raws, kept=kept, fpu_picks=mcts.fpu_picks,
                fpu_unvisited_picks=mcts.fpu_unvisited_picks, vis_wins=list(mcts.vis_wins),
                unv_wins=list(mcts.unv_wins), differs=list(mcts.differs))


def search_counts(seed, env, root, sims, cpuct, r=None, r_root=None, ctr=0):
    """yk_mcts_search of one external root on a fresh tree -> (counts int32[3226], the stream counter after,
    the FpuMCTS)."""
    rs = spec.Stream(seed, env, int(ctr))
    mcts = FpuMCTS(seed, env, rs, sims, cpuct, r, r_root)
    got = mcts.get_action_counts(np.asarray(root, dtype=np.uint64))
    counts = np.zeros(ASIZE, dtype=np.int32)
    for a, c in got.items():
        counts[a] = c
    return counts, rs.ctr, mcts


def arena_game(seed, env, seat, sims, cpuct=1.0, r=None, r_root=None, opponent="random", max_moves=64):
    """Arena.playGame (Arena.py:30-93) for one game on the stream (seed, env): the MCTS agent
    (np.argmax(getActionProb(x, temp=0)), MCTS.py:44-49: the tie pick draws below(len(best))) in seat `seat`
    against RandomYachtPlayer (below(len(legal))) or, opponent="mcts", a second MCTS with its own tree (the
    gating arena's two players).  -> result (curPlayer * getGameEnded), totals, actions, final, ctr, and the two
    counters summed over both players."""
    board, ctr = O.init_board(seed, [env])
    board, rs = board[0], spec.Stream(seed, env, int(ctr[0]))
    players = {seat: FpuMCTS(seed, env, rs, sims, cpuct, r, r_root)}
    if opponent == "mcts":
        players[-seat] = FpuMCTS(seed, env, rs, sims, cpuct, r, r_root)
    cur, actions = 1, []
    while float(O.ended(board, cur)[0][0]) == 0 and len(actions) < max_moves:
        canon = O.canonical(board, cur)[0]
        m = players.get(cur)
        if m is not None:
            counts = m.get_action_counts(canon)
            mx = max(counts.values()) if counts else 0
            if mx == 0:
                action = rs.below(ASIZE)
            else:
                best = [a for a in sorted(counts) if counts[a] == mx]
                action = best[rs.below(len(best))]
        else:
            legal = np.flatnonzero(O.valid(canon, 1)[0][0])
            action = int(legal[rs.below(len(legal))]) if len(legal) else 0
        actions.append(action)
        nxt, npl, st, ctr = O.step(board, cur, action, seed, env, rs.ctr)
        assert st[0] == 0
        rs.ctr = int(ctr[0])
        board, cur = nxt[0], int(npl[0])
    ended, totals = O.ended(board, cur)
    ms = list(players.values())
    return dict(result=float(cur) * float(ended[0]), totals=np.asarray(O.ended(board, 1)[1][0], dtype=np.int32),
                actions=actions, final=board.astype(np.uint64), ctr=rs.ctr,
                fpu_picks=sum(m.fpu_picks for m in ms), fpu_unvisited_picks=sum(m.fpu_unvisited_picks for m in ms))
