"""
Tests that set the library's launch switches (HK_USE_RING, HK_FORCE_GENERAL, HK_WAVE_SLOTS, HK_SEG_BIG, HK_SEG_TAIL,
HK_XCD_REMAP) run on a context of their own: hk_ctx_create reads them, and a context created before they were set never sees them.
"""
import contextlib

import pytest

from homonim_amd import _hk


@contextlib.contextmanager
def launch_context(ctx, env):
    """ `ctx` itself when `env` (name -> value) is empty; otherwise a fresh context on ctx's device, created with `env` set in the
    environment.  The context is closed and the environment restored when the block ends. """
    if not env:
        yield ctx
        return
    with pytest.MonkeyPatch.context() as mp:
        for name, value in env.items():
            mp.setenv(name, value)
        c = _hk.Context(ctx.device, n_streams=1)
        try:
            yield c
        finally:
            c.close()
