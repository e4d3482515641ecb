"""bench.py's command line and result line: a plain run is the default and `--full` opts into everything beyond the headline;
the contract fields of the line are computed the same way in both."""
import pytest

import bench


def test_full_is_opt_in():
    args = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert not args.full
    assert (args.steps, args.warmup, args.gpus) == (7, 2, 1)
    assert bench.parse_args(["--full"]).full


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_result_line_contract_fields():
    args = bench.parse_args(["--steps", "10", "--warmup", "3", "--batch", "4", "--height", "256", "--width", "128", "--precision", "fp8"])
    line = bench.result_line(args, world=2, elapsed=0.05)
    assert line["metric"] == "stereo pairs/sec (enc+dec)"
    assert line["unit"] == "stereo pairs/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(2 * 4 * 10 / 0.05)
    assert line["ms_per_step"] == pytest.approx(5.0)
    assert line["dtype"] == "fp8"
    assert (line["n_gpus"], line["steps"], line["warmup"]) == (2, 10, 3)
    assert (line["config"]["pairs_per_gpu"], line["config"]["height"], line["config"]["width"]) == (4, 256, 128)
