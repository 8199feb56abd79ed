"""No kernel writes outside its output arrays, and none needs them 16-byte aligned.

Every other test allocates `out`, `status` and `error_count` with exactly `count` elements at
the start of a torch allocation, which is 512-B aligned and rounded up to 512 B: a flush that
stores one element too many, or a store that assumes a 16-B aligned output, would land in
slack nobody looks at. Here each output is a slice [5 : 5 + count] of a sentinel-filled int32
tensor of count + 9 words -- 20 bytes in: 4-byte aligned, never 16 -- and the words around it
must still hold the sentinel afterwards. The values inside the slice are checked against the
oracle as everywhere else (a kernel that writes nothing would pass a guard-only test).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from subspace_amd import gpu, slots, synth  # noqa: E402
from test_gpu_base_alignment import flip_tenth, run_strided, slot_sizes  # noqa: E402
from test_gpu_slots import build_channel, offsets  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
M32 = 0xFFFFFFFF
SENTINEL = 0x5EA7B0B5
LEAD, TAIL = 5, 4
COUNTS = [1, 63, 65, 301, 4097]


def guarded(count):
    """(the slice to hand to the library, a function that checks the guard words and returns
    the slice's values as uint32)."""
    full = torch.full((count + LEAD + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
    view = full[LEAD:LEAD + count]
    assert view.data_ptr() % 16 == 4 and view.numel() == count

    def read():
        got = full.cpu().numpy().view(np.uint32)
        before, after = got[:LEAD], got[LEAD + count:]
        assert (before == SENTINEL).all(), f"words before the output overwritten: {before}"
        assert (after == SENTINEL).all(), f"words after the output overwritten: {after}"
        return got[LEAD:LEAD + count].copy()
    return view, read


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("length,stride", [(4096, 4096), (200, 208), (777, 781), (16384, 16384), (5000, 5008)])
def test_uniform_out_guarded(gpu_ctx, oracle, length, stride, count):
    """The 4 KiB kernel, the small kernel (16-B stride FAST and packed-stride), the long kernel's
    final kernel and the ragged final kernel."""
    rng = np.random.default_rng(length + count)
    host = rng.integers(0, 256, (count - 1) * stride + length + 64, dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    out, read = guarded(count)
    gpu_ctx.crc32_uniform(dev, stride, length, count, out)
    torch.cuda.synchronize()
    want = oracle.crc32_batch(host, np.arange(count, dtype=np.uint64) * np.uint64(stride),
                              np.full(count, length, dtype=np.uint64), threads=8)
    assert np.array_equal(read(), want)


def test_ragged_out_guarded(gpu_ctx, oracle):
    rng = np.random.default_rng(700)
    lengths = rng.integers(0, 20000, 700).astype(np.uint64)
    lengths[::9] = rng.integers(0, 300, len(lengths[::9]))
    offs, total = synth.packed_offsets(lengths, 1)
    offs = offs + np.uint64(3)
    host = rng.integers(0, 256, int(total) + 3 + 64, dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    out, read = guarded(700)
    gpu_ctx.crc32_ragged(dev, torch.from_numpy(offs.view(np.int64)).to(DEV),
                         torch.from_numpy(lengths.view(np.int64)).to(DEV), out)
    torch.cuda.synchronize()
    assert np.array_equal(read(), oracle.crc32_batch(host, offs, lengths))


def run_slot_list(ctx, oracle, count, slot_size, bound, cs, ms, sizes, seed, castagnoli=False, status_of=None):
    """Publish, then verify after bit flips, a shuffled device slot list over a channel of
    slot_size-byte slots with max_message_size `bound`: publish byte-identical to the oracle's
    publisher, verify statuses and mismatch count equal to the oracle's subscriber.
    status_of(n): as run_strided's."""
    if status_of is None:
        def status_of(n):
            t = torch.full((n,), 7, dtype=torch.int32, device=DEV)
            return t, lambda: t.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(seed)
    host, ps, stride = build_channel(count, slot_size, cs, ms, sizes, seed=seed + 1)
    host = np.concatenate([host, rng.integers(0, 256, 64, dtype=np.uint8)])
    po, yo = offsets(count, stride, ps)
    dev = torch.from_numpy(host).to(DEV)
    order = rng.permutation(count)
    base = np.uint64(dev.data_ptr())
    rec = slots.slot_records(base + po[order], base + yo[order], sizes[order])
    d_rec = torch.from_numpy(rec.view(np.int64)).to(DEV)
    kw = dict(max_message_size=bound, checksum_size=cs, metadata_size=ms)
    status, read_status = status_of(count)
    ctx.crc32_slots(d_rec, mode=gpu.SLOT_CALCULATE, status=status, **kw)
    torch.cuda.synchronize()
    oracle.publish_slots(host, po, yo, sizes, cs, ms, castagnoli=castagnoli)
    assert (read_status() == 0).all()
    bad = np.nonzero(dev.cpu().numpy() != host)[0]
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:8]} (stride {stride})"
    flip_tenth(host, po, yo, sizes, rng)
    want = oracle.verify_slots(host, po[order], yo[order], sizes[order], cs, ms, castagnoli=castagnoli)
    dev.copy_(torch.from_numpy(host))  # same addresses: the records stay valid
    status, read_status = status_of(count)
    err, read_err = status_of(1)
    ctx.crc32_slots(d_rec, mode=gpu.SLOT_VERIFY, status=status, error_count=err, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(read_status(), want)
    assert int(read_err()[0]) == int((want == 1).sum()) > 0
    assert np.array_equal(dev.cpu().numpy(), host)  # verify never writes the channel


# (slot size, max_message_size, metadata_size, payload sizes from .. to): full 4 KiB payloads
# (FAST waves), short ones (the waves repack), the packed forms, the unfused finish (small
# kernel + crc32_slot_finish_kernel), and the ragged pipeline + slot finish (bound 32,768, the
# payloads of up to 12,000 B in slots of that size: 4,097 of them are about 50 MB)
SLOT_LISTS = {
    "4k-full": (4096, 4096, 0, 4096, 4096),
    "4k-short": (4096, 4096, 0, 0, 500),
    "256": (256, 256, 0, 0, 256),
    "4k-meta100": (4096, 4096, 100, 0, 4096),
    "32k": (12000, 32768, 0, 1, 12000),
}


def slot_list_sizes(name, count):
    lo, hi = SLOT_LISTS[name][3:]
    return np.random.default_rng(count + hi).integers(lo, hi + 1, count).astype(np.uint64)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", list(SLOT_LISTS))
def test_slot_list_status_guarded(gpu_ctx, oracle, name, count):
    slot_size, bound, ms = SLOT_LISTS[name][:3]
    run_slot_list(gpu_ctx, oracle, count, slot_size, bound, 4, ms, slot_list_sizes(name, count),
                  seed=count * 11 + bound + ms, status_of=guarded)


@pytest.mark.parametrize("count", COUNTS)
def test_strided_fused_4k_status_guarded(gpu_ctx, oracle, count):
    """The fused 4 KiB slot kernel's status and mismatch-count stores."""
    run_strided(gpu_ctx, oracle, count, 4096, 4, 0, None, 0, seed=count + 4, status_of=guarded)


@pytest.mark.parametrize("count", COUNTS)
def test_strided_sizes_1000_status_guarded(gpu_ctx, oracle, count):
    """The fused small-slot kernel over a strided channel with per-slot sizes."""
    run_strided(gpu_ctx, oracle, count, 1000, 4, 0, slot_sizes(count, 1000, count), 0, seed=count + 1000,
                status_of=guarded)
