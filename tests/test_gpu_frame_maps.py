"""The maps of a frame whose replicas do not all take part (pt_frame_preview, pt_frame_get_noise, pt_frame_get_variance,
pt_frame_preview_measured): three replicas over two tiles that leave half of the image uncovered, so that one
replica's entries are gathered on replica 0's own device, one's come by way of the host and one replica owns nothing.  Every map equals
the one-replica frame's over the same tiles bit for bit.  Every call is limited to whole passes, so nothing here depends on a clock."""
import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

SIDE = 32
SEED = 4711
QUANTUM = 16


def _maps(frame):
    raw, samples = frame.preview()
    denoised, denoised_samples = frame.preview(denoise=True)
    measured, measured_samples = frame.preview_measured()
    return {"preview": raw, "preview samples": samples, "denoised preview": denoised, "denoised preview samples": denoised_samples,
            "error map": frame.error_map(), "variance": frame.variance(), "measured preview": measured, "measured preview samples": measured_samples}


def test_three_replicas_two_tiles_against_one_replica():
    sc, cam = scenes.cornell_scene(SIDE, SIDE)
    opt = scenes.options(SIDE, SIDE, 8, 64)
    tiles = np.array([(0, 0, 16, 16), (16, 0, 16, 16)], binding.TILE_DTYPE)
    covered = np.zeros((SIDE, SIDE), bool)
    covered[:16] = True
    gpus = [binding.Scene(sc, device=0) for _ in range(4)]
    frames = []
    try:
        many = binding.Frame(gpus[:3], cam, opt, base_seed=SEED, tiles=tiles)  # (tile k goes to replica k: replica 2 owns nothing)
        frames.append(many)
        one = binding.Frame(gpus[3], cam, opt, base_seed=SEED, tiles=tiles)
        frames.append(one)
        for k in range(2):
            what = "after %d passes" % (k + 1)
            for frame in frames:
                frame.set_progressive(QUANTUM, 1)
                assert frame.render()[2]["status"] == binding.PT_ERR_CANCELLED, what
            got, want = _maps(many), _maps(one)
            samples = got["preview samples"]
            print("%s: %d + %d unfinished pixels in the two tiles, %d finished" % (what, (samples[:16, :16] > 0).sum(), (samples[:16, 16:] > 0).sum(),
                                                                                 (samples == -1).sum()))
            assert (samples[:16, :16] > 0).any() and (samples[:16, 16:] > 0).any(), what + ": both replicas that own a tile have entries"
            for name in want:
                assert_bits_equal(got[name], want[name], "%s, %s: three replicas against one" % (what, name))
            noise, want_noise = many.noise(), one.noise()
            assert set(noise) == set(want_noise)
            for key in want_noise:
                assert np.array_equal(np.asarray(noise[key]), np.asarray(want_noise[key])), "%s, noise()[%r]: %s against %s" % (what, key, noise[key], want_noise[key])
            assert noise["streams_total"] == 2 * 16 * 16 and noise["streams_rated"] + noise["streams_unrated"] == (samples > 0).sum(), what
            assert (samples[covered] != 0).all(), what + ": every covered pixel is finished or has samples"
            assert (samples[~covered] == 0).all() and (got["preview"][~covered] == 0).all(), what + ": uncovered pixels are holes"
            assert np.isposinf(got["error map"][~covered]).all(), what + ": uncovered pixels of the error map"
            assert (got["variance"][~covered] == 0).all(), what + ": uncovered pixels of the variance map"
        images = []
        for frame in frames:
            frame.set_progressive(0)
            image, tile_done, info = frame.render()
            assert info["status"] == binding.PT_OK and tile_done.all() and frame.done
            images.append(image)
        assert_bits_equal(images[0], images[1], "the finished frames")
        assert (images[0][~covered] == 0).all()
    finally:
        for frame in frames:
            frame.close()
        for gpu in gpus:
            gpu.close()
