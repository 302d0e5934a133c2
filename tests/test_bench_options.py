"""bench.py's command line: a plain run is the headline alone; --full and --dump-outputs are off unless given."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_outputs_are_off_by_default():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.steps == 5 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"
