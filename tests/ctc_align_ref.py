"""Host references of the CTC forced alignment (include/tavsr.h, tavsr_ctc_align): a numpy restatement of the recursion with
the same tie rule (float64 by default), a brute-force enumerator over every frame labelling, and the helpers the tests share."""
import itertools

import numpy as np


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def collapse(labels, blank=0):
    """merge repeats, drop blank"""
    out, prev = [], None
    for c in labels:
        c = int(c)
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def feasible(Tb, target, V, blank=0):
    target = [int(c) for c in target]
    if any(c < 0 or c >= V or c == blank for c in target):
        return False
    return Tb >= len(target) + sum(target[i] == target[i - 1] for i in range(1, len(target)))


def align_ref(lp, Tb, target, blank=0, T=None, Lmax=None, dtype=np.float64):
    """lp [>= Tb, V] log-probabilities of one utterance -> (align int64 [T], frame_lp [T], span int32 [Lmax, 2], score, path
    int [Tb]); an infeasible problem gives (-1, 0, -1, -inf, [])."""
    lp = np.asarray(lp, dtype=dtype)
    V = lp.shape[1]
    T = lp.shape[0] if T is None else T
    L = len(target)
    Lmax = L if Lmax is None else Lmax
    Tb = max(0, min(int(Tb), T))
    align = np.full(T, -1, np.int64)
    frame_lp = np.zeros(T, dtype)
    span = np.full((Lmax, 2), -1, np.int32)
    if not feasible(Tb, target, V, blank):
        return align, frame_lp, span, -np.inf, []
    if Tb == 0:
        return align, frame_lp, span, 0.0, []
    S = 2 * L + 1
    lab = [blank if s % 2 == 0 else int(target[s // 2]) for s in range(S)]
    ninf = dtype(-np.inf)
    d = np.full(S, ninf, dtype)
    d[0] = lp[0, blank]
    if S > 1:
        d[1] = lp[0, lab[1]]
    moves = np.zeros((Tb, S), np.int8)
    lab_a = np.array(lab)
    skip = np.zeros(S, bool)      # move 2 exists: s odd, s >= 3 and lab(s) != lab(s-2)
    skip[3::2] = lab_a[3::2] != lab_a[1:-2:2]
    for t in range(1, Tb):      # all states at once; the candidates in the order 0, 1, 2 with a strict >
        d1 = np.concatenate(([ninf], d[:-1]))
        d2 = np.where(skip, np.concatenate(([ninf, ninf], d[:-2]))[:S], ninf)
        best, mv = d.copy(), np.zeros(S, np.int8)
        m1 = d1 > best
        best[m1], mv[m1] = d1[m1], 1
        m2 = d2 > best
        best[m2], mv[m2] = d2[m2], 2
        moves[t] = mv
        with np.errstate(invalid="ignore"):
            d = np.where(best == ninf, ninf, best + lp[t, lab_a]).astype(dtype)
    s = S - 2 if S >= 2 and d[S - 2] > d[S - 1] else S - 1
    score = float(d[s])
    path = [0] * Tb
    path[Tb - 1] = s
    for t in range(Tb - 1, 0, -1):
        s -= int(moves[t, s])
        path[t - 1] = s
    for t, s in enumerate(path):
        align[t] = lab[s]
        frame_lp[t] = lp[t, lab[s]]
    span[:L] = spans_of_path(path, L)
    return align, frame_lp, span, score, path


def spans_of_path(path, L):
    """[L, 2]: first frame in state 2l+1 and last such frame + 1 (-1 where the state is never visited)"""
    span = np.full((L, 2), -1, np.int32)
    for t, s in enumerate(path):
        if s % 2 == 1:
            if span[s // 2, 0] < 0:
                span[s // 2, 0] = t
            span[s // 2, 1] = t + 1
    return span


def spans_of_align(align, Tb, target, blank=0):
    """the spans that an alignment (frame labels) implies for ``target``: runs of non-blank labels, in order; None when the
    alignment does not collapse to the target"""
    runs, prev = [], blank
    for t in range(Tb):
        c = int(align[t])
        if c != blank and c != prev:
            runs.append([c, t, t + 1])
        elif c != blank:
            runs[-1][2] = t + 1
        prev = c
    if [r[0] for r in runs] != [int(c) for c in target]:
        return None
    return np.array([[r[1], r[2]] for r in runs], np.int32).reshape(len(runs), 2)


def path_score(lp, align, Tb):
    """float64 log-probability of a frame labelling"""
    lp = np.asarray(lp, np.float64)
    return float(sum(lp[t, int(align[t])] for t in range(Tb)))


def brute_force(lp, Tb, target, blank=0):
    """best score over all V^Tb frame labellings that collapse to the target (-inf when there is none); float64"""
    lp = np.asarray(lp, np.float64)
    V = lp.shape[1]
    target = [int(c) for c in target]
    if Tb == 0:
        return 0.0 if not target else -np.inf
    best = -np.inf
    for labels in itertools.product(range(V), repeat=Tb):
        if collapse(labels, blank) == target:
            best = max(best, sum(lp[t, c] for t, c in enumerate(labels)))
    return float(best)


def random_state_path(rng, Tb, target, blank=0):
    """a random valid state path of ``Tb`` frames through the lattice of ``target`` (list of states), or None if infeasible"""
    L = len(target)
    S = 2 * L + 1
    lab = [blank if s % 2 == 0 else int(target[s // 2]) for s in range(S)]
    # need[s]: fewest frames that still reach an end state from s (s included)
    need = [0] * S
    for s in range(S - 1, -1, -1):
        if s >= S - 2:
            need[s] = 1
        else:
            nxt = [need[s + 1]]
            if s + 2 < S and (s + 2) % 2 == 1 and lab[s + 2] != lab[s]:
                nxt.append(need[s + 2])
            need[s] = 1 + min(nxt)
    starts = [s for s in (0, 1) if s < S and need[s] <= Tb]
    if not starts or Tb == 0:
        return None
    s = int(rng.choice(starts))
    path = [s]
    for t in range(1, Tb):
        left = Tb - t
        cand = [s]
        if s + 1 < S:
            cand.append(s + 1)
        if s + 2 < S and (s + 2) % 2 == 1 and lab[s + 2] != lab[s]:
            cand.append(s + 2)
        cand = [c for c in cand if need[c] <= left]
        s = int(rng.choice(cand))
        path.append(s)
    return path


def planted(seed, T, L, V, blank=0, boost=12.0, repeat=0.3):
    """N(0,1) logits [T, V] plus ``boost`` on a random valid state path of a random target with about ``repeat`` repeated
    tokens -> (logits fp32, target list, path list)"""
    rng = np.random.default_rng(seed)
    target = []
    for i in range(L):
        if i and rng.random() < repeat:
            target.append(target[-1])
        else:
            target.append(int(rng.integers(1, V)) if blank == 0 else int(rng.integers(0, V - 1)))
    while True:
        path = random_state_path(rng, T, target, blank)
        if path is not None:
            break
        i = int(rng.integers(1, L))      # too many repeats for T frames: break one
        target[i] = (target[i - 1] % (V - 1)) + 1
    logits = rng.standard_normal((T, V)).astype(np.float32)
    for t, s in enumerate(path):
        logits[t, blank if s % 2 == 0 else target[s // 2]] += np.float32(boost)
    return logits, target, path
