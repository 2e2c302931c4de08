"""Engine.options and Engine.profiled: what a block changes comes back, whatever ends the block.  No kernel runs."""
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("max_work_bytes", "seed_chan_stride", "harm_eps", "profile")


def test_option_blocks_restore_what_they_found():
    from pulseportraiture_amd.engine import Engine, EngineError
    e = Engine(0)
    try:
        before = {n: e.get_option(n) for n in NAMES}
        with pytest.raises(ZeroDivisionError):
            with e.options(max_work_bytes=1e6, profile=1):
                with e.options(seed_chan_stride=0, harm_eps=0.0, max_work_bytes=2e6):      # (the stride is clamped to 1)
                    assert [e.get_option(n) for n in NAMES] == [2e6, 1.0, 0.0, 1.0]
                    1 / 0
        assert {n: e.get_option(n) for n in NAMES} == before
        # blocks that end normally, nested: the inner one restores the outer one's value
        with e.options(seed_chan_stride=8):
            with e.options(seed_chan_stride=0):
                assert e.get_option("seed_chan_stride") == 1.0
            assert e.get_option("seed_chan_stride") == 8.0
        assert {n: e.get_option(n) for n in NAMES} == before
        # an unknown name raises before anything is changed
        with pytest.raises(EngineError):
            with e.options(max_work_bytes=1e6, no_such_option=1):
                raise AssertionError("the block was entered")
        assert {n: e.get_option(n) for n in NAMES} == before
        for was in (0, 1):
            with e.options(profile=was):
                with e.profiled() as kt:
                    assert e.get_option("profile") == 1.0 and kt == {}
                assert isinstance(kt, dict) and e.get_option("profile") == was
        assert {n: e.get_option(n) for n in NAMES} == before
    finally:
        e.close()
