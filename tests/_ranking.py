"""The one judge of a reranked query answer (a plain helper module: imported by the tests, collected by nobody).

`judge_ranking` compares an answer - a list of (id, score) - with the reference flow's answer for the same query AND
with the truth it can compute itself: the float64 cosine of every candidate's row *as stored* (what `fetch` returns: for
a 16- or 8-bit corpus the stored form, which is what those tests hand the oracle too).  The reference's own order among
near-ties is unspecified, so position-by-position agreement of ids cannot be asked; what can be asked is that every id
carries ITS score, that the order is the scores' order, and that nothing better was left out.

`literal_lists` is dict counting over BucketCSR segments: the model of the candidate kernels.
"""

from __future__ import annotations

import numpy as np


class RankingMismatch(AssertionError):
    """An answer the judge refuses; `check` is the number (1 .. 5) of the check that fired."""

    def __init__(self, check, message):
        super().__init__(f"check {check}: {message}")
        self.check = check


def cosines_f64(query, rows):
    """cos(query, row) for every row, in float64 from the float32 values handed in."""
    q = np.asarray(query, dtype=np.float32).reshape(-1).astype(np.float64)
    x = np.asarray(rows, dtype=np.float32).astype(np.float64).reshape(-1, q.shape[0])
    return (x @ q) / (np.linalg.norm(x, axis=1) * np.linalg.norm(q))


def judge_ranking(got, want, *, query, candidates, fetch, tol=1e-5, gap=2e-5):
    """got, want: lists of (id, score) - the answer under test and the literal flow's (oracle.query_literal with top_p).
    candidates: the literal flow's candidate ids for `query` (query_literal(..., top_k=None)); fetch: ids -> rows as stored.

    1. Equal lengths; position by position the scores agree within `tol` where the ids agree, and within `tol + gap`
       where they do not (near-ties of the reference; a tie may straddle the cut).
    2. The ids are distinct, and all of them are candidates.
    3. Every score is its id's float64 cosine with `query`, within `tol`.
    4. The scores are non-increasing, exactly, as the float32 values returned.
    5. The cut is complete: a candidate left out has a float64 cosine <= min(returned scores) + tol.  (Derived: the
       score the device gave a left-out candidate is at most the last kept score, and within `tol` of its truth.)
       Skipped when nothing is left out.
    """
    got = [(int(i), float(s)) for i, s in got]
    want = [(int(i), float(s)) for i, s in want]
    # 1
    if len(got) != len(want):
        raise RankingMismatch(1, f"{len(got)} entries, the reference has {len(want)}")
    for j, ((gi, gs), (wi, ws)) in enumerate(zip(got, want)):
        if gi == wi:
            if not abs(gs - ws) <= tol:
                raise RankingMismatch(1, f"position {j}, id {gi}: score {gs!r}, the reference's {ws!r}")
        elif not abs(gs - ws) <= tol + gap:
            raise RankingMismatch(1, f"position {j}: id {gi} with {gs!r} where the reference has id {wi} with {ws!r}")
    # 2
    cand = [int(c) for c in candidates]
    allowed = set(cand)
    seen = {}
    for j, (gi, _) in enumerate(got):
        if gi in seen:
            raise RankingMismatch(2, f"position {j}: id {gi} was already returned at position {seen[gi]}")
        seen[gi] = j
        if gi not in allowed:
            raise RankingMismatch(2, f"position {j}: id {gi} is not a candidate of this query")
    if not got:
        if cand:
            raise RankingMismatch(5, f"nothing returned of {len(cand)} candidates")
        return
    # 3
    truth = dict(zip(cand, cosines_f64(query, fetch(cand)).tolist()))
    for j, (gi, gs) in enumerate(got):
        if not abs(gs - truth[gi]) <= tol:
            raise RankingMismatch(3, f"position {j}, id {gi}: score {gs!r}, its cosine is {truth[gi]!r}")
    # 4
    for j in range(1, len(got)):
        if not got[j - 1][1] >= got[j][1]:
            raise RankingMismatch(4, f"position {j}, id {got[j][0]}: score {got[j][1]!r} above {got[j - 1][1]!r} "
                                     f"of id {got[j - 1][0]} before it")
    # 5
    floor = min(s for _, s in got)
    for c in cand:
        if c not in seen and not truth[c] <= floor + tol:
            raise RankingMismatch(5, f"id {c} with cosine {truth[c]!r} was left out; the last kept score is {floor!r}")


def literal_lists(segments, keys, nb, bb):
    """Per query: [(id, collisions)] ordered by (-collisions, id) - dict counting over the buckets the keys select, an id
    once per band however many segments list it there."""
    out = []
    for qi in range(keys.shape[0]):
        counts = {}
        for b in range(nb):
            code = (b << (8 * bb)) | int.from_bytes(keys[qi, b].tobytes(), "little")
            members = set()
            for seg in segments:
                g = int(np.searchsorted(seg.codes, code))
                if g < len(seg) and int(seg.codes[g]) == code:
                    members.update(seg.members[seg.offsets[g]:seg.offsets[g + 1]].tolist())
            for m in members:
                counts[m] = counts.get(m, 0) + 1
        out.append(sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])))
    return out
