"""tests/_ranking.judge_ranking bites: the reference's own answer (oracle.top_k_cosine, cut as LSHRS.query cuts) passes
at every cut, exact duplicate vectors included; every way an answer can be wrong with its scores still plausible raises,
from the check that is there for it.  No GPU."""

from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import lshrs_oracle as O
from tests._ranking import RankingMismatch, cosines_f64, judge_ranking

TOL = 1e-5
DIM = 48


def _rows_with_cosines(rng, query, cosines):
    """One float32 row per wanted cosine with `query`, of random length."""
    q = query.astype(np.float64) / np.linalg.norm(query.astype(np.float64))
    rows = []
    for c in cosines:
        u = rng.standard_normal(len(q))
        u -= (u @ q) * q
        u /= np.linalg.norm(u)
        rows.append((c * q + math.sqrt(1.0 - c * c) * u) * rng.uniform(0.5, 3.0))
    return np.asarray(rows, dtype=np.float32)


def _case(seed=0, n=400, duplicates=0):
    """ids (sparse, unordered), their rows, a query, the reference's full ranking.  The cosines are spread so that
    neighbours in the ranking are 1e-3 or more apart (the mutations that need a near-tie use `_near_ties`)."""
    rng = np.random.default_rng(seed)
    query = rng.standard_normal(DIM).astype(np.float32)
    cos = np.linspace(0.95, -0.6, n) + rng.uniform(-1e-3, 1e-3, n)
    rows = _rows_with_cosines(rng, query, cos)
    if duplicates:
        src = rng.choice(n, duplicates, replace=False)
        rows = np.concatenate([rows, rows[src]])                      # exact copies: equal scores, either one may be cut
    ids = rng.permutation(10 * len(rows))[:len(rows)].astype(np.int64) + 7
    table = {int(i): r for i, r in zip(ids, rows)}
    fetch = lambda want: np.stack([table[int(i)] for i in want])  # noqa: E731
    ranked = [(int(ids[p]), s) for p, s in O.top_k_cosine(query, rows, k=len(rows))]
    return query, ids.tolist(), fetch, ranked


def _cut(ranked, top_p, top_k=None):
    return ranked[:O.expected_limit(len(ranked), top_p, top_k)]


@pytest.mark.parametrize("duplicates", [0, 60])
@pytest.mark.parametrize("top_p,top_k", [(1.0, None), (0.5, None), (0.01, None), (0.3, 5), (1.0, 3), (1e-9, None)])
def test_the_references_own_answer_passes(top_p, top_k, duplicates):
    for seed in range(4):
        query, cand, fetch, ranked = _case(seed, duplicates=duplicates)
        want = _cut(ranked, top_p, top_k)
        judge_ranking(list(want), want, query=query, candidates=cand, fetch=fetch)
        worst = max(abs(s - t) for (_, s), t in zip(want, cosines_f64(query, fetch([i for i, _ in want]))))
        assert worst <= 1e-6                                          # (the f32 reference against float64: far inside tol)


def test_duplicates_straddling_the_cut_pass_either_way():
    """Two exact copies on either side of the cut: the answer may keep either one."""
    rng = np.random.default_rng(3)
    query = rng.standard_normal(DIM).astype(np.float32)
    rows = _rows_with_cosines(rng, query, np.linspace(0.9, 0.1, 20))
    rows[10] = rows[9]
    ids = list(range(100, 120))
    fetch = lambda want: rows[np.asarray(want) - 100]  # noqa: E731
    ranked = [(ids[p], s) for p, s in O.top_k_cosine(query, rows, k=20)]
    want = ranked[:10]
    assert {want[9][0], ranked[10][0]} == {109, 110} and want[9][1] == ranked[10][1]
    other = want[:9] + [ranked[10]]
    judge_ranking(want, want, query=query, candidates=ids, fetch=fetch)
    judge_ranking(other, want, query=query, candidates=ids, fetch=fetch)


def _near_ties(seed=11):
    """A case whose ranking has, by construction, pairs of neighbours 1.5e-5 and 2.5e-5 apart (more than `tol`, within the
    `tol + gap` = 3e-5 that check 1 allows where ids differ): positions (4, 5) are 1.5e-5 apart, and position 30 - the cut used
    below keeps 30 entries - is 2.5e-5 below position 29.  Everything else is 1e-3 or more apart."""
    rng = np.random.default_rng(seed)
    query = rng.standard_normal(DIM).astype(np.float32)
    cos = np.linspace(0.9, 0.3, 60)
    cos[5] = cos[4] - 1.5e-5
    cos[30] = cos[29] - 2.5e-5
    rows = _rows_with_cosines(rng, query, cos)
    ids = (rng.permutation(1000)[:60] + 1).tolist()
    table = {i: r for i, r in zip(ids, rows)}
    fetch = lambda want: np.stack([table[int(i)] for i in want])  # noqa: E731
    ranked = [(ids[p], s) for p, s in O.top_k_cosine(query, rows, k=60)]
    assert [i for i, _ in ranked] == ids                              # the construction's order is the ranking's
    assert 1.2e-5 < ranked[4][1] - ranked[5][1] < 1.8e-5 and 2.2e-5 < ranked[29][1] - ranked[30][1] < 2.8e-5
    return query, ids, fetch, ranked


def _rotate_ids(want, full):
    ids = [i for i, _ in want]
    return [(i, s) for i, (_, s) in zip(ids[1:] + ids[:1], want)]


def _non_candidate(want, full):
    out = list(want)
    out[7] = (10 ** 9, out[7][1])
    return out


def _duplicate_id(want, full):
    out = list(want)
    out[8] = (out[7][0], out[8][1])
    return out


def _drop_a_better_one(want, full):
    # the last kept entry gives way to the next one in the ranking, 2.5e-5 below it: more than 2 * tol, yet within the tol + gap
    # check 1 allows where ids differ.  The entry that moves in carries ITS cosine and the order holds: only the cut is wrong.
    return list(want[:-1]) + [full[len(want)]]


def _score_off_same_id(want, full):
    out = list(want)
    out[12] = (out[12][0], out[12][1] + 3 * TOL)
    return out


def _score_off_behind_a_tie_swap(want, full):
    # positions 4 and 5 are 1.5e-5 apart: an answer may hold them the other way round, and check 1 then allows tol + gap at both.
    # The id now at 5 is given a score 3 * tol below its cosine: 1.5e-5 from the reference's at that position, and still in order.
    out = list(want)
    out[4], out[5] = want[5], (want[4][0], want[4][1] - 3 * TOL)
    return out


def _swap_adjacent(want, full):
    out = list(want)
    out[4], out[5] = out[5], out[4]                                   # 1.5e-5 apart: check 1 lets a near-tie swap through
    return out


@pytest.mark.parametrize("mutate,check,why", [
    (_rotate_ids, 3, "ids rotated under unchanged scores: every position has the reference's score, no id has its own"),
    (_non_candidate, 2, "an id no bucket of the query holds, under the reference's score"),
    (_duplicate_id, 2, "an id twice, under the reference's scores"),
    (_drop_a_better_one, 5, "a candidate 2.5e-5 better than the last one kept is left out: more than 2 * tol"),
    (_score_off_same_id, 1, "an agreeing id's score 3 * tol off the reference's: what the position-by-position check always caught"),
    (_score_off_behind_a_tie_swap, 3, "a score 3 * tol off where the ids differ: within check 1's tol + gap, so only check 3 - the id's own cosine - can see it; "
                                      "where the ids agree a wrong score never reaches check 3, check 1 has it first"),
    (_swap_adjacent, 4, "two neighbours 1.5e-5 apart in the wrong order: ids and scores all right, the order not"),
], ids=lambda v: v.__name__.strip("_") if callable(v) else None)
def test_every_mutation_raises_from_its_check(mutate, check, why):
    query, cand, fetch, ranked = _near_ties()
    want = ranked[:30]
    judge_ranking(list(want), want, query=query, candidates=cand, fetch=fetch)
    bad = mutate(want, ranked)
    assert bad != want
    with pytest.raises(RankingMismatch) as info:
        judge_ranking(bad, want, query=query, candidates=cand, fetch=fetch)
    assert info.value.check == check, (why, str(info.value))


def test_a_short_or_long_answer_raises_from_check_1():
    query, cand, fetch, ranked = _near_ties()
    want = ranked[:30]
    for bad in (want[:-1], ranked[:31]):
        with pytest.raises(RankingMismatch) as info:
            judge_ranking(bad, want, query=query, candidates=cand, fetch=fetch)
        assert info.value.check == 1


def test_the_long_list_gap_widens_check_1_only():
    """`gap=1e-4` (the near-copies of the long-list test) lets ids differ where scores are 1e-4 apart; a rotated answer on
    spread-out data still fails - from check 3, whose tolerance `gap` does not touch."""
    query, cand, fetch, ranked = _case(5)
    want = _cut(ranked, 0.5)
    with pytest.raises(RankingMismatch) as info:
        judge_ranking(_rotate_ids(want, ranked), want, query=query, candidates=cand, fetch=fetch, gap=1e-4)
    assert info.value.check == 3
