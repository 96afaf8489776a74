"""The encoder cases tests/test_video_gpu.py runs on the device, with what each is for; tests/test_video_cpu.py
asserts on the twin alone that every input does what it is for."""
import numpy as np


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def cases():
    """name -> (image [H,W,3] uint8, quality)"""
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    step = np.zeros((8, 16, 3), dtype=np.uint8)
    step[:, 8:] = 255
    # p = 16 (-1)^(x+y) in every channel: at quality 50 only the last coefficient of Y survives the quantisation (the issue's
    # amplitude 80 leaves a dozen small ones in front of it and no run of 16 zeros: the input was adjusted, not the assertion)
    checker = np.repeat((128 + 16 * (-1) ** (x + y)).astype(np.uint8)[:, :, None], 3, axis=2)
    return {"a: one MCU": (noise(8, 8, 1), 90),
            "b: padding both ways, two segments": (noise(20, 12, 2), 90),
            "c: ten segments": (noise(8, 80, 3), 90),
            "d: one segment of 384 blocks": (noise(1024, 8, 4), 100),
            "e: white": (np.full((16, 16, 3), 255, dtype=np.uint8), 90),
            "f: a step from 0 to 255": (step, 100),
            "g: the highest frequency alone": (checker, 50)}


def assert_exercises(name, stats):
    """`jpeg_twin.symbol_stats` of a case's file shows what the case is for."""
    k = name[0]
    if k == "a":
        assert stats["markers"] == []
    elif k == "b":
        assert stats["markers"] == [0xD0]
    elif k == "c":
        assert len(stats["markers"]) == 9 and stats["markers"].count(0xD0) == 2          # the markers wrap past RST7
    elif k == "d":
        assert stats["markers"] == [] and stats["stuffed"] >= 1
    elif k == "e":
        assert stats["ac_category"] == 0 and stats["zrl"] == 0
    elif k == "f":
        assert stats["dc_category"] == 11
    elif k == "g":
        assert stats["zrl"] >= 1
    else:
        raise KeyError(name)
