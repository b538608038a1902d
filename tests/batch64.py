"""The pair sizes of the B = 64 tests of the ragged point-cloud ops (knn, rigid, segment, selfsup, ground).

A workgroup finds its pair by a six-step search whose first step (32) is taken only in batches of 33 to 64 pairs.  The sizes
cycle through 0, 1, 3, 37, 300 with empty pairs at the batch's ends and around that step (0, 31, 32, 33, 63), and pairs 40 and
50 span several workgroups at either span in use (256 and 1024 points), so that past the step the workgroup prefix and the
pair index differ by a changing amount.  7 180 points in all."""

CYCLE = (0, 1, 3, 37, 300)
EMPTY = (0, 31, 32, 33, 63)
LARGE = {40: 2100, 50: 1025}


def counts64():
    counts = [CYCLE[i % len(CYCLE)] for i in range(64)]
    for i in EMPTY:
        counts[i] = 0
    for i, n in LARGE.items():
        counts[i] = n
    return counts


def prefix_of(counts):
    prefix = [0]
    for n in counts:
        prefix.append(prefix[-1] + n)
    return prefix
