"""The profiling window the route tests open around their calls (test infrastructure): the launch
families the library records between codec_profile_begin and codec_profile_end, by the names of
_lib.KERNEL_TAGS -- one tag per route, whatever the template arguments.  Shared by
tests/test_pee_launch_variants.py (every instantiation behind a knob, two slices) and
tests/test_pee_batch_dispatch.py (no knob, the batch sizes at which the dispatch changes route)."""
import contextlib


@contextlib.contextmanager
def launches(seen, capacity=64):
    """adds the launch families (profiling tags) recorded inside the block to `seen`; a window holds
    `capacity` launches and must not overflow (a launch past it would go unrecorded)"""
    import ctypes as C
    import torch
    from codec_tcc_amd import _lib
    lib = _lib.load()
    _lib.check(lib.codec_profile_begin(capacity), "codec_profile_begin")
    n = -1
    try:
        yield
    finally:
        torch.cuda.synchronize()
        tags = (C.c_int32 * capacity)()
        n = lib.codec_profile_end(None, tags, capacity)
        seen.update(_lib.KERNEL_TAGS.get(tags[i], str(tags[i])) for i in range(max(n, 0)))
    assert 0 <= n < capacity, f"the profiling window of {capacity} launches is full: widen it"
