"""All five sample-quality metrics in one short training run: the schedule (rcgan_amd.metrics.Evaluations) on the real evaluators.
Periods 2 / 4 / 2 / 4 / 2 over 4 iterations, the smallest sizes the flag checks allow."""
import os
import re

import pytest

from tests.train_launch import launch

pytestmark = pytest.mark.gpu

TITLES = ["frechet distance", "manifold precision and recall", "kernel distance", "intra-class msssim", "nearest training images"]
FLAGS = ["--frechet_freq", "2", "--prdc_freq", "4", "--kid_freq", "2", "--msssim_freq", "4", "--neighbours_freq", "2",
         "--kid_subset_size", "64", "--msssim_pairs", "20"]
for _p in ("frechet", "prdc", "kid", "msssim", "neighbours"):
    FLAGS += ["--%s_samples" % _p, "200", "--%s_real_samples" % _p, "1024"]


def test_every_metric_runs_at_its_period_in_table_order_on_one_classifier(tmp_path):
    text, built = launch(tmp_path, FLAGS, "all5")
    started = re.findall(r"INFO\s+starting calculating (.*)\.$", text, flags=re.M)
    assert started == [TITLES[0], TITLES[2], TITLES[4]] + TITLES + TITLES, text[-3000:]       # iteration 1, iteration 3, the end
    assert re.findall(r"INFO\s+finished calculating (.*)\.$", text, flags=re.M) == started
    assert built == 1
    for line in (r"frechet real statistics: 1024 images, computed", r"manifold real set: 1024 images, k = 5, label classifier shared",
                 r"kernel distance real set: 1024 images, label classifier shared", r"msssim real set: 1024 images, 20 pairs per class, intra-class ",
                 r"neighbours real set: 1024 training images, 10000 held-out images, held-out copy rate "):
        assert len(re.findall(r"INFO\s+" + re.escape(line), text)) == 1, line
    for name in ("neighbours_1.png", "neighbours_3.png", "neighbours_final.png"):
        assert os.path.exists(os.path.join(str(tmp_path), "all5", name)), name
