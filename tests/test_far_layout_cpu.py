""" The far layouts and the arena checksum of tests/_far_layout.py, without a device: every narrowing of an offset of these
layouts stays inside the used part of the arena (so a kernel that narrows shows as wrong bytes, not as a fault), a narrowed
offset of a far plane is never the true one (so it does show), and the expected checksum equals a direct sum, wrap included. """
import numpy as np
import pytest

import _far_layout as fl

# (itemsize, layout kind, planes F apart): what tests/test_gpu_far_planes.py places -- 8-byte samples never take the 3-row form
FORMS = [(1, 'band', 2), (2, 'band', 2), (4, 'band', 2), (8, 'band', 2), (1, 'row', 3), (2, 'row', 3), (4, 'row', 3), (8, 'row', 2)]


@pytest.mark.parametrize('delta', list(fl.DELTAS.values()), ids=list(fl.DELTAS))
@pytest.mark.parametrize('itemsize, kind, planes', FORMS, ids=[f'{k}{p}x{i}B' for i, k, p in FORMS])
def test_every_narrowing_lands_inside_the_used_arena_and_off_the_true_pixel(delta, itemsize, kind, planes):
    lay = fl.Layout(kind, delta)
    h, w, pitch = (planes, 1100, 1100) if kind == 'row' else (37, 261, 264)
    shape = (1, h, w) if kind == 'row' else (planes, h, w)
    stride, band_stride = lay.strides(h, pitch)
    end = max(lay.extent(k, shape, pitch) for k in range(fl.MAX_ARRAYS)) * itemsize
    used = fl.used_bytes(end)
    assert used <= fl.ARENA_BYTES
    assert used > (1 << 32) * itemsize   # the far plane is further than 32 bits of bytes AND of elements
    for k in (0, fl.MAX_ARRAYS - 1):
        base = fl.slot(k, delta)
        for band in range(shape[0]):
            for y in sorted({0, h - 1}):
                for x in (0, w - 1):
                    true = (base + band * band_stride + y * stride + x) * itemsize
                    reached = fl.narrowings(base, band, band_stride, y, stride, x, itemsize)
                    assert true in reached
                    for off in reached:
                        assert 0 <= off and off + itemsize <= used, (k, band, y, x, off)
                    is_far = (band if kind == 'band' else y) > 0
                    if is_far:
                        # whatever is narrowed -- the far term, the sum or the bytes -- the pixel reached is another one, and it lies
                        # behind every array's first plane or row: on the canary, or on a nearer far plane
                        wrong = reached - {true}
                        assert len(wrong) >= 1 and all(o < true for o in wrong)
                        assert min(wrong) >= (base + x) * itemsize
                    else:
                        assert reached == {true}
    # the first planes of all arrays lie in front of what a narrowed F leaves, so a narrowed far access never hits an input's start
    assert fl.slot(fl.MAX_ARRAYS - 1, delta) + delta // 8 <= delta


def test_odd_delta_aligns_no_far_plane_and_aligned_delta_every_one():
    for itemsize in (1, 2, 4):
        for j in (1, 2):
            assert (j * fl.far(fl.DELTA_ODD) * itemsize) % 16 != 0
    assert (fl.far(fl.DELTA_ODD) * 8) % 16 != 0
    assert all((j * fl.far(fl.DELTA_ALIGNED) * it) % 16 == 0 for j in (1, 2) for it in (1, 2, 4, 8))
    assert fl.far(fl.DELTA_ODD) % 4 != 0 and fl.far(fl.DELTA_ALIGNED) % 4 == 0


def test_the_largest_forms_fit_the_arena():
    for delta in fl.DELTAS.values():
        assert fl.used_bytes(fl.Layout('row', delta).extent(fl.MAX_ARRAYS - 1, (1, 3, 1100), 1100) * 4) <= fl.ARENA_BYTES
        assert fl.used_bytes(fl.Layout('row', delta).extent(1, (1, 2, 70), 70) * 8) <= fl.ARENA_BYTES
        assert fl.used_bytes(fl.Layout('band', delta).extent(fl.MAX_ARRAYS - 1, (2, 20, 40), 40) * 8) <= fl.ARENA_BYTES
    with pytest.raises(AssertionError):   # the form that is left out: three float64 rows
        fl.used_bytes(fl.Layout('row', fl.DELTA_ALIGNED).extent(0, (1, 3, 70), 70) * 8)


def _direct_sum(buf):
    return sum(int(v) for v in buf.view('<u4').tolist()) % (1 << 64)


def test_the_expected_checksum_equals_a_direct_sum_on_a_small_arena():
    rng = np.random.default_rng(3)
    used = 3 * fl.CHUNK + 512   # (not a whole number of the model's pieces)
    fake = np.full(used, fl.CANARY, np.uint8)
    model = fl.ArenaModel(used)
    assert model.checksum() == _direct_sum(fake) == (used // 4) * fl.CANARY_WORD
    writes = [(0, 16), (5, 3), (fl.CHUNK - 2, 7), (2 * fl.CHUNK + 1, fl.CHUNK + 100), (used - 9, 9), (6, 1), (1000, 0)]
    for off, n in writes:   # unaligned, across pieces, overlapping, up to the last byte, empty
        data = rng.integers(0, 256, n, dtype=np.uint8)
        fake[off:off + n] = data
        model.write(off, data)
        assert model.checksum() == _direct_sum(fake)
    assert model.read(0, used).tobytes() == fake.tobytes()
    typed = rng.normal(size=(3, 5)).astype(np.float32)   # an array goes in as its bytes
    model.write(256, typed)
    fake[256:256 + typed.nbytes] = np.frombuffer(typed.tobytes(), np.uint8)
    assert model.checksum() == _direct_sum(fake)
    with pytest.raises(AssertionError):
        model.write(used - 3, np.zeros(4, np.uint8))


def test_the_expected_checksum_wraps_modulo_2_64():
    used = fl.ARENA_BYTES
    n_words = used // 4
    model = fl.ArenaModel(used)
    assert n_words * fl.CANARY_WORD >= 1 << 64   # the canary alone wraps
    assert model.checksum() == (n_words * fl.CANARY_WORD) % (1 << 64) != n_words * fl.CANARY_WORD
    # words far apart, the last one of the arena among them: against the sum written out with Python's integers
    rng = np.random.default_rng(4)
    total = n_words * fl.CANARY_WORD
    for off in (0, (1 << 34) + 4, used - 4):
        word = rng.integers(0, 1 << 32, 1, dtype=np.uint64).astype('<u4')
        model.write(off, word)
        total += int(word[0]) - fl.CANARY_WORD
    assert model.checksum() == total % (1 << 64)
    # a direct sum over a small window in front of a canary remainder that wraps
    small = np.full(8192, fl.CANARY, np.uint8)
    data = rng.integers(0, 256, 5000, dtype=np.uint8)
    small[100:5100] = data
    model = fl.ArenaModel(used)
    model.write(100, data)
    assert model.checksum() == (_direct_sum(small) + (n_words - small.size // 4) * fl.CANARY_WORD) % (1 << 64)


def test_rows_and_strides_of_the_layouts():
    f = fl.far(fl.DELTA_ODD)
    assert fl.Layout('band', fl.DELTA_ODD).strides(37, 264) == (264, f)
    assert fl.Layout('row', fl.DELTA_ODD).strides(3, 264) == (f, 3 * f)
    assert fl.Layout('compact').strides(37, 264, 8) == (264, 37 * 264 + 8)
    runs = fl.row_runs((2, 2, 5), 4, fl.slot(1, fl.DELTA_ODD), 8, f)
    base = fl.DELTA_ODD // 8
    assert runs == [(4 * base, 0, 0), (4 * (base + 8), 0, 1), (4 * (base + f), 1, 0), (4 * (base + f + 8), 1, 1)]
