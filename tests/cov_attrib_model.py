"""The attribution walk of wtfgpu_attribute_coverage, restated (a test checker).

`sets[i]` is the live new-coverage set of the lane at position i of the list,
`revoke[i]` marks a timed-out testcase, `aggregate` is the device aggregate at
the call. A testcase reports the values no earlier testcase committed
(bochscpu_backend.cc:499-505); a timed-out one reports but does not commit
(client.cc:120-126)."""
from __future__ import annotations


def attribute(sets, revoke=None, aggregate=(), full=False):
    """[(pos, v)] sorted by (pos, v)."""
    revoke = [False] * len(sets) if revoke is None else list(revoke)
    assert len(revoke) == len(sets)
    have = set(aggregate)
    out = []
    for i, s in enumerate(sets):
        for v in sorted(set(s)):
            if full:  # parity mode: no filter, no first-owner rule
                out.append((i, v))
                continue
            if v in have:
                continue
            out.append((i, v))
            if not revoke[i]:
                have.add(v)
    return out
