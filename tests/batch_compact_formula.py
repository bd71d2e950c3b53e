"""What ``RunStats.image_launches`` must be after ``BatchEngine.run_until_stable``:
a pure function of the loop's arguments and of the check at which each image
converged, shared by test_batch_compact_cpu.py (hand-made cases) and
test_gpu_batch_compact.py (the engine).

The loop: chunks of ``check_every`` repetitions (the last one shorter), each
``ceil(chunk / fuse)`` fused launches; after chunk j comes check j, and chunk
j + 1 is enqueued before check j's counts are read.  The loop ends at the check
after which no image is open, or when ``max_reps`` leaves no further chunk.

With compaction an image that converged at check j is in the grids of chunks
1 .. j + 1 (the chunk in flight while check j was read still carries it), or of
every chunk made if there are fewer; an image that never converged is in every
chunk.  Without compaction every image is in every chunk."""
import math


def chunk_launches(max_reps, check_every, fuse, converged_at):
    """Fused launches of each chunk the loop makes.  ``converged_at[b]``: the
    1-based check at which image b converged, ``None`` if it never did."""
    done = min(check_every, max_reps)
    chunks, checks = [done], 0
    while True:
        nxt = min(check_every, max_reps - done)
        if nxt > 0:
            chunks.append(nxt)
        checks += 1
        still_open = any(j is None or j > checks for j in converged_at)
        if not still_open or nxt == 0:
            break
        done += nxt
    return [math.ceil(x / fuse) for x in chunks]


def expected_image_launches(max_reps, check_every, fuse, converged_at, compact):
    """(image_launches, launches) of one run_until_stable over len(converged_at) images."""
    per_chunk = chunk_launches(max_reps, check_every, fuse, converged_at)
    launches = sum(per_chunk)
    if not compact:
        return launches * len(converged_at), launches
    total = 0
    for j in converged_at:
        upto = len(per_chunk) if j is None else min(j + 1, len(per_chunk))
        total += sum(per_chunk[:upto])
    return total, launches


def converged_at(infos):
    """The formula's input from a list of StableInfo."""
    return [i.checks if i.converged else None for i in infos]
