"""generate_images.py end to end on the GPU: a tiny random checkpoint carrying ``generator_ema``, a pooled text
embedding from a file (no CLIP weights), each run in a fresh child process.  The PNG has the reference's name
(<prompt with spaces as underscores>.png) and the reference's size: a one-row figure of 4 x 4 inch panels at
matplotlib's default 100 dpi, 400 * num_samples x 400 pixels.  ``--ema`` must sample other weights than the
default run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(REPO, "moe-gan_cpsc541_amd")
CHILD = ("import sys, matplotlib; matplotlib.rcdefaults(); import generate_images; "
         "generate_images.main(sys.argv[1:])")


def _generate(args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG]), MPLBACKEND="Agg")
    r = subprocess.run([sys.executable, "-c", CHILD] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_generate_images_writes_the_reference_png(tmp_path):
    import t2i_moe_gan as M
    from PIL import Image
    G, G_ema = M.AuroraGenerator(seed=21), M.AuroraGenerator(seed=22)
    ck = os.path.join(tmp_path, "ck.pt")
    torch.save({"generator": G.state_dict(), "discriminator": M.AuroraDiscriminator(seed=23).state_dict(),
                "generator_ema": G_ema.state_dict()}, ck)
    emb = os.path.join(tmp_path, "text.npy")
    np.save(emb, torch.randn(1, 512, generator=torch.Generator().manual_seed(5)).numpy())
    prompt = "a red bus on a street"
    common = ["--checkpoint", ck, "--prompt", prompt, "--text_embedding", emb, "--num_samples", "2", "--seed", "1"]
    pixels = {}
    for name, extra in (("ema", ["--ema"]), ("live", [])):
        out_dir = os.path.join(tmp_path, name)
        log = _generate(common + ["--output_dir", out_dir] + extra)
        png = os.path.join(out_dir, "a_red_bus_on_a_street.png")
        assert os.path.exists(png), log
        assert os.listdir(out_dir) == ["a_red_bus_on_a_street.png"]
        with Image.open(png) as im:
            assert im.size == (800, 400)
            pixels[name] = np.asarray(im.convert("RGB")).copy()
        assert "Warning" not in log
    assert not np.array_equal(pixels["ema"], pixels["live"])
