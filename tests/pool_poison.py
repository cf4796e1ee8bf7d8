"""Poisoned-pool runs: the instrument that shows a kernel reading memory nobody wrote.

Every workspace and output of the device modules is a torch.empty (the library allocates nothing itself).  Fresh device memory is usually zero and
recycled memory usually holds a plausible earlier activation, so a read of an element no kernel wrote passes every parity test -- until another job
leaves something else behind.  Here the caching allocator's free memory is filled with a byte pattern first, the stage under test then builds its
module and runs out of that memory alone, and the same stage is run under several patterns: outputs that differ between patterns (or hold a NaN)
depend on unwritten memory.

    poison(pattern, large_bytes, n_small) -> the allocator's device-allocation count afterwards
    sizes(stage)                          -> (large_bytes, n_small) from one unpoisoned dry run of the stage
    pattern_dependence(stage)             -> [] or the list of findings, one line each

A pattern may be listed twice: two runs under the SAME pattern that differ show a result that changes from run to run whatever the memory held (every
run builds its module anew and finds its buffers at other addresses), which is a finding of its own kind and must not be taken for an unwritten read.

The condition that makes a run mean something: between poison() and the end of the run the allocator obtained NO new memory from the driver
(device_allocations() unchanged) -- everything the stage allocated was poisoned memory.  pattern_dependence asserts it; it is a condition on the run,
not a measurement of the stage.

A plain helper module (imported by tests/test_gpu_pool_poison.py), not a conftest: it changes nothing about how any other test runs."""
import gc

import torch

PATTERNS = (0x00, 0xFF, 0x7F)        # zeros | NaN as float, -1 as int32 | 3.39e38 as float, a large positive int32
SMALL = 512 * 1024                   # <= 1 MB: served from the allocator's small-block pool (2 MB segments)
MIN_LARGE = 128 << 20                # the 64 MB verification block must fit the large block whatever the stage needs
VERIFY = (4 << 10, 512 << 10, 4 << 20, 64 << 20)


def device_allocations():
    """how often the caching allocator has obtained a segment from the driver so far"""
    return int(torch.cuda.memory_stats()["num_device_alloc"])


def _sweep(held):
    """Segments that live tensors of other tests pin cannot be released by empty_cache, and their free fragments would be handed out unpoisoned.  Take
    blocks of every size class, largest first, for as long as the allocator serves them WITHOUT new memory; the one block per class that does open a new
    segment is kept too (it is poisoned with the rest).  Appends to `held`."""
    size = 32 << 20
    while size >= 512:
        for _ in range(4096):
            before = device_allocations()
            held.append(torch.empty(size, dtype=torch.uint8, device="cuda"))
            if device_allocations() != before:
                break
        size //= 2


def poison(pattern_byte, large_bytes, n_small):
    """Fill the allocator's free memory with `pattern_byte`: one block of large_bytes, n_small blocks of 512 KB (the small-block pool) and the free
    fragments of pinned segments; free all of it back to the cache; verify that fresh torch.empty tensors of 4 KB, 512 KB, 4 MB and 64 MB consist of
    the pattern only and cost no new segment.  Returns device_allocations() afterwards."""
    assert 0 <= pattern_byte <= 0xFF and large_bytes >= MIN_LARGE
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = []
    _sweep(held)
    held.append(torch.empty(large_bytes, dtype=torch.uint8, device="cuda"))
    held += [torch.empty(SMALL, dtype=torch.uint8, device="cuda") for _ in range(n_small)]
    for t in held:
        t.fill_(pattern_byte)
    torch.cuda.synchronize()
    del t
    held.clear()
    count = device_allocations()
    for nbytes in VERIFY:
        probe = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        host = probe.cpu()
        del probe
        assert bool((host == pattern_byte).all()), f"poison 0x{pattern_byte:02X} did not take: a fresh {nbytes}-byte block holds something else"
    assert device_allocations() == count, "the verification blocks were not served from the poisoned cache"
    return count


def sizes(stage):
    """(large_bytes, n_small) for `stage`: twice the peak of one unpoisoned dry run, overall and of the small-block pool"""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    s0 = torch.cuda.memory_stats()
    out = stage()
    torch.cuda.synchronize()
    del out
    s1 = torch.cuda.memory_stats()
    peak = s1["allocated_bytes.all.peak"] - s0["allocated_bytes.all.current"]
    small = s1["allocated_bytes.small_pool.peak"] - s0["allocated_bytes.small_pool.current"]
    return max(2 * int(peak), MIN_LARGE), 2 * int(small) // SMALL + 8


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.numel() else t


def findings(runs, patterns=PATTERNS):
    """runs: one {name: host tensor} per pattern -> the names whose bits differ between patterns or that hold a NaN, one line each"""
    found = []
    for name, first in runs[0].items():
        for i, (pat, run) in enumerate(zip(patterns, runs)):
            t = run[name]
            if t.is_floating_point() and bool(torch.isnan(t).any()):
                found.append(f"{name}: {int(torch.isnan(t).sum())} NaN under 0x{pat:02X}")
            if t.shape != first.shape or not torch.equal(_bits(t), _bits(first)):
                n = "shape" if t.shape != first.shape else int((t != first).sum())
                found.append(f"{name}: run {i} (0x{pat:02X}) differs from run 0 (0x{patterns[0]:02X}) ({n} elements)")
    return found


def pattern_dependence(stage, patterns=PATTERNS):
    """stage() builds what it needs on the device, runs, and returns {name: tensor} holding only what the interface specifies (a tail the header
    leaves open is the stage's to cut off).  -> findings (empty: the outputs do not depend on what the memory held before)"""
    large_bytes, n_small = sizes(stage)
    runs = []
    for pat in patterns:
        count = poison(pat, large_bytes, n_small)
        out = stage()
        torch.cuda.synchronize()
        host = {k: v.detach().cpu() for k, v in out.items()}
        del out
        assert device_allocations() == count, (f"under 0x{pat:02X} the run obtained new memory from the driver ({device_allocations() - count} segments, "
                                               f"large block {large_bytes >> 20} MB, {n_small} small blocks): the run proves nothing")
        runs.append(host)
    return findings(runs, patterns)
