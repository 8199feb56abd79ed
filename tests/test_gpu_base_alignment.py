"""GPU parity with a `dev_base` that is not on a 16-byte boundary.

Every other GPU test passes the start of a torch allocation (512-B aligned) and produces
misalignment through strides, offsets and slot addresses only. Here the base pointer itself
is moved by k bytes (k = 1, 8, 15; k = 0 once per shape as the control), which
 * turns off the host's `dev_base % 16` decisions in subspace_crc32_batch_uniform (the 4 KiB
   kernel, the long kernel, the small kernel's 16-B-stride FAST form) and in
   subspace_crc32_slots_strided (the fused slot kernel, the `aligned` flag), and
 * makes every 128-bit load unaligned: the kernels round offsets *relative to the base*
   (`base + (s & ~15)`), so a block boundary is k bytes off a 16-B address.
Inputs are numpy-random bytes uploaded to the device and the expected values come from the
oracle over the host copy, so nothing depends on the device fill generator. Every buffer
keeps at least 64 allocated bytes after the last message byte (base offsets stay below 16, so
block-rounded reads relative to a moved base stay inside the tensor). All comparisons are
bit-exact.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from subspace_amd import _lib, gpu, synth  # noqa: E402
from test_gpu_slots import build_channel, offsets  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
M32 = 0xFFFFFFFF
KS = [0, 1, 8, 15]
INIT2 = 0x12345678  # the non-default init, used together with finalize=True
SLACK = 16 + 64     # the largest base offset + the bytes kept after the last message byte


def run_uniform(ctx, oracle, length, stride, count, k, seed, crc_batch=None):
    """Message i = host[k + i*stride :][:length]; one call with the default init (raw state)
    and one with INIT2 and finalize, each equal to the oracle over the host copy."""
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, (count - 1) * stride + length + SLACK, dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 16 == 0
    offs = np.uint64(k) + np.arange(count, dtype=np.uint64) * np.uint64(stride)
    lens = np.full(count, length, dtype=np.uint64)
    crc_batch = crc_batch or oracle.crc32_batch
    for init, finalize in ((M32, False), (INIT2, True)):
        out = torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        ctx.crc32_uniform(dev, stride, length, count, out, init=init, finalize=finalize, base_offset=k)
        torch.cuda.synchronize()
        want = crc_batch(host, offs, lens, init)
        if finalize:
            want = want ^ np.uint32(M32)
        got = out.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (f"length {length} stride {stride} count {count} base+{k} init {init:#x}: "
                               f"{len(bad)} wrong, first at {bad[:8]}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("length,stride", [(4096, 4096), (4096, 4160)])
def test_uniform_4k_base_offset(gpu_ctx, oracle, length, stride, k):
    """crc32_uniform4k_kernel when the base is aligned; materialised offsets + the ragged
    path otherwise (4096 + 15 extended bytes do not fit the small kernel)."""
    run_uniform(gpu_ctx, oracle, length, stride, 257, k, seed=length + stride + k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("length,stride", [(16384, 16384), (8192, 8208)])
def test_uniform_long_base_offset(gpu_ctx, oracle, length, stride, k):
    """Whole 8 KiB pieces: crc32_long_kernel when the base is aligned, the ragged path otherwise."""
    run_uniform(gpu_ctx, oracle, length, stride, 37, k, seed=length + stride + k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("count", [301, 4097])
@pytest.mark.parametrize("length,stride", [(64, 64), (200, 208), (1000, 1008), (2048, 2048), (4081, 4096),
                                           (777, 781)])
def test_uniform_small_base_offset(gpu_ctx, oracle, length, stride, count, k):
    """The small-message kernel: the 16-B-stride FAST form when base and stride are aligned,
    the packed-stride form (chosen because of the base, crc_small.hip `ua`) otherwise; 777/781
    is packed either way. 4,097 messages give several tiles per wave and a partial last tile."""
    run_uniform(gpu_ctx, oracle, length, stride, count, k, seed=length * 7 + count + k)


@pytest.mark.parametrize("k", KS)
def test_uniform_4090_base_offset(gpu_ctx, oracle, k):
    """4,090 bytes fit the small kernel's half-tile only from an aligned base (4,081 otherwise)."""
    run_uniform(gpu_ctx, oracle, 4090, 4096, 301, k, seed=4090 + k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("length,stride", [(5000, 5008), (8191, 8192)])
def test_uniform_materialised_base_offset(gpu_ctx, oracle, length, stride, k):
    """Shapes that take materialised offsets + the ragged path whatever the base."""
    run_uniform(gpu_ctx, oracle, length, stride, 37, k, seed=length + k)


@pytest.mark.parametrize("k", [0, 15])
@pytest.mark.parametrize("length", [1, 100, 4096])
def test_uniform_single_message(gpu_ctx, oracle, length, k):
    """count == 1 with a length of at most 4 KiB: the dispatcher's `count > 1` test sends it to
    the ragged path (4096 from an aligned base: the 4 KiB kernel with one message)."""
    run_uniform(gpu_ctx, oracle, length, length, 1, k, seed=length + k)


@pytest.mark.parametrize("k", [0, 15])
def test_uniform_zero_stride_zero_length(gpu_ctx, k):
    """stride == 0 with length == 0: every result is init ^ final_xor."""
    dev = torch.zeros(SLACK, dtype=torch.uint8, device=DEV)
    for init, finalize in ((M32, False), (INIT2, True)):
        out = torch.full((5,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        gpu_ctx.crc32_uniform(dev, 0, 0, 5, out, init=init, finalize=finalize, base_offset=k)
        torch.cuda.synchronize()
        want = init ^ (M32 if finalize else 0)
        assert (out.cpu().numpy().view(np.uint32) == np.uint32(want)).all()


# ------------------------------------------------------------------ ragged API
_RAGGED = {}


def ragged_batch():
    """About 700 messages packed at align=1 behind a random lead: empty, 1..300 bytes, every
    8192*j + d around a tile boundary, and up to 70,000 bytes (host bytes, offsets, lengths)."""
    if not _RAGGED:
        rng = np.random.default_rng(0xBA5E)
        edge = [8192 * j + d for j in range(1, 5) for d in (-17, -16, -1, 0, 1, 15, 16, 17)]
        lengths = np.concatenate([np.zeros(20, dtype=np.int64), rng.integers(1, 301, 400), np.array(edge),
                                  rng.integers(301, 70001, 700 - 420 - len(edge))]).astype(np.uint64)
        rng.shuffle(lengths)
        offs, total = synth.packed_offsets(lengths, 1)
        offs = offs + np.uint64(rng.integers(1, 16))
        end = int((offs + lengths).max())
        host = rng.integers(0, 256, end + SLACK, dtype=np.uint8)
        _RAGGED.update(host=host, offsets=offs, lengths=lengths, end=end)
    return _RAGGED


def run_ragged(ctx, k, fused_prep, exact_arena, want, init=INIT2):
    """The batch of ragged_batch() read from base = buf[k:], and the same bytes through the
    aligned base with offsets + k; both must equal `want`."""
    b = ragged_batch()
    dev = torch.from_numpy(b["host"]).to(DEV)
    assert dev.data_ptr() % 16 == 0
    n = len(b["lengths"])
    d_off = torch.from_numpy(b["offsets"].view(np.int64)).to(DEV)
    d_offk = torch.from_numpy((b["offsets"] + np.uint64(k)).view(np.int64)).to(DEV)
    d_len = torch.from_numpy(b["lengths"].view(np.int64)).to(DEV)
    moved = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    plain = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    dev_lib = _lib.load_dev()
    assert dev_lib.subspace_crc_testutil_set(ctx._h, b"fused_prep", fused_prep) == 0
    try:
        ctx.crc32_ragged(dev[k:], d_off, d_len, moved, init=init, finalize=True,
                         arena_bytes=b["end"] if exact_arena else None)
        ctx.crc32_ragged(dev, d_offk, d_len, plain, init=init, finalize=True,
                         arena_bytes=b["end"] + k if exact_arena else None)
        torch.cuda.synchronize()
    finally:
        dev_lib.subspace_crc_testutil_set(ctx._h, b"fused_prep", 1)
    moved = moved.cpu().numpy().view(np.uint32)
    plain = plain.cpu().numpy().view(np.uint32)
    bad = np.nonzero(moved != want)[0]
    assert len(bad) == 0, f"base+{k}: {len(bad)} wrong, first at {bad[:8]}, lengths {b['lengths'][bad[:8]]}"
    # the same bytes from the aligned base: a failure above then names the base, not the batch
    assert np.array_equal(plain, want)


@pytest.mark.parametrize("exact_arena", [True, False])
@pytest.mark.parametrize("fused_prep", [1, 0])
@pytest.mark.parametrize("k", KS)
def test_ragged_base_offset(gpu_ctx, oracle, k, fused_prep, exact_arena):
    """subspace_crc32_batch from a moved base: the descriptors' tile starts, the buffer
    resources built on base + tile start and the tile counts are all relative to the base; with
    the fused tile-count + descriptor kernel and the separate kernels, the arena given exactly
    and as the whole tensor."""
    b = ragged_batch()
    want = oracle.crc32_batch(b["host"], b["offsets"] + np.uint64(k), b["lengths"], INIT2) ^ np.uint32(M32)
    run_ragged(gpu_ctx, k, fused_prep, exact_arena, want)


# ------------------------------------------------------------------ strided slots at 8 mod 16
def flip_tenth(host, po, yo, sizes, rng):
    """One bit flipped in a tenth of the slots (at least one): in the payload, or in the stored
    checksum of an empty one."""
    count = len(po)
    for i in rng.choice(count, max(1, count // 10), replace=False):
        n = int(sizes[i])
        at = int(yo[i]) + int(rng.integers(0, n)) if n else int(po[i]) + 48
        host[at] ^= np.uint8(1 << int(rng.integers(0, 8)))


def run_strided(ctx, oracle, count, slot_size, cs, ms, sizes, k, seed, castagnoli=False, status_of=None):
    """Publish, then verify after bit flips, a contiguous channel whose buffer starts k bytes
    into the tensor. sizes None: uniform messages of slot_size bytes. Publish: the whole
    device tensor, lead and slack included, equals the oracle-published host copy; verify:
    statuses and the mismatch count equal oracle.verify_slots. status_of(n) -> (tensor to pass,
    function returning its uint32 values after checking whatever surrounds it)."""
    if status_of is None:
        def status_of(n):
            t = torch.full((n,), 7, dtype=torch.int32, device=DEV)
            return t, lambda: t.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(seed)
    uniform = sizes is None
    osizes = np.full(count, slot_size, dtype=np.uint64) if uniform else sizes
    chan, ps, stride = build_channel(count, slot_size, cs, ms, osizes, seed=seed + 1)
    host = rng.integers(0, 256, k + len(chan) + 64, dtype=np.uint8)
    host[k:k + len(chan)] = chan
    po, yo = offsets(count, stride, ps)
    po, yo = po + np.uint64(k), yo + np.uint64(k)
    dev = torch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 16 == 0
    d_sizes = None if uniform else torch.from_numpy(sizes.view(np.int64)).to(DEV)
    kw = dict(message_size=slot_size if uniform else 0, sizes=d_sizes, checksum_size=cs, metadata_size=ms,
              base_offset=k)
    status, read_status = status_of(count)
    ctx.crc32_slots_strided(dev, stride, count, mode=gpu.SLOT_CALCULATE, status=status, **kw)
    torch.cuda.synchronize()
    oracle.publish_slots(host, po, yo, osizes, cs, ms, castagnoli=castagnoli)
    assert (read_status() == 0).all()
    bad = np.nonzero(dev.cpu().numpy() != host)[0]
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:8]} (stride {stride}, base+{k})"
    flip_tenth(host, po, yo, osizes, rng)
    want = oracle.verify_slots(host, po, yo, osizes, cs, ms, castagnoli=castagnoli)
    dev.copy_(torch.from_numpy(host))
    status, read_status = status_of(count)
    err, read_err = status_of(1)
    ctx.crc32_slots_strided(dev, stride, count, mode=gpu.SLOT_VERIFY, status=status, error_count=err, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(read_status(), want)
    assert int(read_err()[0]) == int((want == 1).sum()) > 0
    assert np.array_equal(dev.cpu().numpy(), host)  # verify never writes the channel


def slot_sizes(count, slot_size, seed):
    sizes = np.random.default_rng(seed).integers(0, slot_size + 1, count).astype(np.uint64)
    if count >= 3:
        sizes[:3] = [0, 1, slot_size]
    else:
        sizes[0] = slot_size - 3
    return sizes


@pytest.mark.parametrize("count", [1, 1501])
@pytest.mark.parametrize("cs,ms", [(4, 0), (4, 16)])
def test_strided_uniform_4k_buffer_8_mod_16(gpu_ctx, oracle, cs, ms, count):
    """4 KiB messages at stride 4,160 (no metadata) and 4,224 (16 B of metadata) in a buffer at
    8 mod 16, which the header allows: the fused slot kernel needs 16-B aligned payloads, so the
    payload CRCs come from the uniform call with a misaligned base, then the slot finish."""
    run_strided(gpu_ctx, oracle, count, 4096, cs, ms, None, 8, seed=cs + ms + count)


@pytest.mark.parametrize("count", [1, 1501])
@pytest.mark.parametrize("slot_size,cs,ms", [(1000, 4, 0), (1000, 4, 100), (8192, 4, 0)])
def test_strided_sizes_buffer_8_mod_16(gpu_ctx, oracle, slot_size, cs, ms, count):
    """Per-slot sizes in a buffer at 8 mod 16: 1000-B slots through the fused small kernel (no
    metadata) and the small kernel + slot finish (100 B of metadata), 8192-B slots through the
    ragged path."""
    run_strided(gpu_ctx, oracle, count, slot_size, cs, ms, slot_sizes(count, slot_size, slot_size + ms), 8,
                seed=slot_size + ms + count)
