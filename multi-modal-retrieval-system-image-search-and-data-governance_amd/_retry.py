"""The capacity-and-retry protocol of the calls whose answer has an open size: range search and the self-join, the deep
top-k, the threshold sweep, the decision masks, the assignment (search.py) and the hash joins (dedup.py).  Pure Python, no
tensor and no library: tests/test_capacity_retry_host.py runs it, and its six callers, without a GPU."""


def run(launch, caps, ceiling, overflow, too_big, needed=lambda caps, counts: counts[-1:]):
    """``launch(*caps)`` once, and once more at larger capacities if its counts ask for them.  -> the counts that fit.

    Such a C call runs at fixed capacities, stores nothing past them and reports in ``counts`` what it would have needed
    (include/mmr.h).  ``launch(*caps)`` makes one call at these capacities, allocating what depends on them, and reads
    ``counts`` once.  ``needed(caps, counts)`` gives the capacities those counts call for, one per entry of ``caps``
    (default: one capacity, whose exact count comes last).  A list that overflowed starves the list it feeds (range
    search's candidates its matches, the deep top-k's tiles its survivors), whose count is then an undercount:
    ``needed`` sizes that list by its bound instead.
    * The attempt fits iff every needed size is within its capacity; a first attempt that fits is the whole cost.
    * Otherwise there is one retry, at the larger of capacity and need, entry by entry -- unless some entry of the need
      exceeds ``ceiling`` (the caller's ``max_pairs`` / ``max_ambiguous``): MemoryError(``too_big(needed)``), no allocation.
    * The retry's sizes are exact or upper bounds, so a second overflow is a bug: RuntimeError(``overflow(counts, caps)``).
    """
    for attempt in range(2):
        counts = launch(*caps)
        need = needed(caps, counts)
        if all(n <= c for n, c in zip(need, caps)):
            return counts
        if attempt == 1:
            raise RuntimeError(overflow(counts, caps))
        if max(need) > ceiling:
            raise MemoryError(too_big(need))
        caps = tuple(max(c, n) for c, n in zip(caps, need))
