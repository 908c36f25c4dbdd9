#!/usr/bin/env python3
"""Every *_workspace_bytes query of the C ABI over a grid, one JSON line per answer: two builds of the library that state the same
workspace layouts print the same file.  The handle-free queries (ResNet trunk with a null net, GRU, dwconv_same, PPO) run on the host:
HOST_GRID is what tests/test_workspace_layout_host.py pins.  The MobileNetV2 / EfficientNet / shifted-trunk queries need a net object and
with it a device: (n, size, tsm_segments / pad_size, dtype) on both sides of each network's chunk and half-chunk thresholds, and the
"mbv2_chunk" / "effnet_chunk" options at a non-default value.
Usage: python tools/workspace_sizes.py [--host] > sizes.jsonl        (ADAF_LIB=<other build> for the other side; compare with cmp)"""
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import _lib  # noqa: E402

BATCH, STEPS, HIDDEN = (1, 33), (1, 63, 64, 65), (16, 1024)      # steps: both sides of the backward's barrier rounding


def _grid(*axes):
    return list(itertools.product(*axes))


def _gru_backward():       # classes: 5 and one above 3 * hidden (the column-sum partials then follow the classes)
    return [(b, t, h, c) for b, t, h in _grid(BATCH, STEPS, HIDDEN) for c in (5, 3 * h + 1)]


def _dwconv_same():        # (n, h, w, c, k, stride, dtype): 7 and 1001 pixels (1 x 7, 7 x 143), square maps of the EfficientNet walk, both dtypes
    maps = ((1, 7), (7, 143), (9, 9), (48, 48))
    return [(n, h, w, c, k, s, d) for n, (h, w), c, k, s, d in _grid(BATCH, maps, (16, 1280), (3, 5), (1, 2), (0, 1))] + \
        [(0, 9, 9, 16, 3, 1, 0), (2, 0, 9, 16, 3, 1, 0), (2, 9, -1, 16, 3, 1, 0), (2, 9, 9, 0, 3, 1, 0), (2, 9, 9, 16, 3, 0, 0)]


# query -> argument tuples; the last tuples of each have a non-positive extent (the answer is 0)
HOST_GRID = {
    "adaf_resnet50_workspace_bytes": [(None, n, p) for n, p in _grid(BATCH, (32, 96, 144))] + [(None, 0, 96), (None, 4, 0)],
    "adaf_gru_cls_workspace_bytes": _grid(BATCH, STEPS, HIDDEN) + [(0, 8, 16), (2, 0, 16), (2, 8, -16)],
    "adaf_gru_cls_train_workspace_bytes": _grid(BATCH, STEPS, HIDDEN) + [(-1, 8, 16), (2, 0, 16), (2, 8, 0)],
    "adaf_gru_cls_backward_workspace_bytes": _gru_backward() + [(0, 8, 16, 5), (2, 0, 16, 5), (2, 8, 0, 5), (2, 8, 16, 0)],
    "adaf_dwconv_same_workspace_bytes": _dwconv_same(),
    "adaf_ppo_head_workspace_bytes": _grid(STEPS, BATCH) + [(0, 4), (4, -1)],
    # (pixels, channels, conv_out): channels % 128 != 0 or conv_out != 32 -> no split-K term
    "adaf_ppo_wenc_grad_workspace_bytes": _grid((7, 1001), (96, 128, 1280), (16, 32)) + [(0, 128, 32), (7, 0, 32), (7, 128, 0)],
    # (steps, batch, map_pixels, channels, conv_out, hidden)
    "adaf_ppo_encoder_backward_workspace_bytes": _grid((1, 65), BATCH, (7, 49), (96, 1280), (32,), HIDDEN) +
    [(0, 2, 49, 1280, 32, 16), (4, 0, 49, 1280, 32, 16), (4, 2, 0, 1280, 32, 16), (4, 2, 49, -128, 32, 16), (4, 2, 49, 1280, 0, 16),
     (4, 2, 49, 1280, 32, 0)],
}


def host_sizes(lib):
    """[(query, args, bytes)] over HOST_GRID."""
    return [(q, args, int(getattr(lib, q)(*args))) for q, grid in HOST_GRID.items() for args in grid]


def emit(query, args, value, **ctx):
    print(json.dumps(dict(query=query, args=[a for a in args if a is not None], bytes=int(value), **ctx), sort_keys=True), flush=True)


def device_sizes(lib):
    import torch
    from adafocus_amd import hip_ops
    dev = torch.device("cuda:0")
    mb = hip_ops.MobileNetV2Net(dev)
    # chunk 512 (default): one chunk, a pair of halves from 512 frames, whole chunks above; clips of 8 / 12 / 16 frames round the chunk
    for chunk in (512, 96):
        with _lib.option("mbv2_chunk", chunk):
            for n, size, T in _grid((1, 33, 95, 96, 97, 192, 193, 480, 511, 512, 513, 528, 1024, 1025, 1536), (32, 96, 128, 224), (0, 8, 12, 16)):
                if T == 0 or n % T == 0:
                    emit("adaf_mobilenetv2_workspace_bytes", (n, size, T), lib.adaf_mobilenetv2_workspace_bytes(mb._net, n, size, T), mbv2_chunk=chunk)
    for name, width, depth in (("b0", 1.0, 1.0), ("b3", 1.2, 1.4)):
        ef = hip_ops.EffNetNet(dev, width, depth)
        for dtype in ("f32", "f16"):
            ef.set_dtype(dtype)
            for chunk in (1024, 48):
                with _lib.option("effnet_chunk", chunk):
                    for n, size, pad in _grid((1, 33, 47, 48, 49, 96, 97, 511, 512, 513, 1023, 1024, 1025, 2048, 2049), (31, 32, 96, 144, 224), (0, 224, 300)):
                        emit("adaf_effnet_workspace_bytes", (n, size, pad), lib.adaf_effnet_workspace_bytes(ef._net, n, size, pad), net=name, dtype=dtype,
                             effnet_chunk=chunk)
        del ef
    trunk = hip_ops.ResNet50Trunk(dev)
    for place in ("blockres", "block"):      # 'block': a sixth slab for the shifted block input
        trunk.set_shift_place(place)
        for n, p in _grid(BATCH, (32, 96, 144)):
            emit("adaf_resnet50_workspace_bytes", (n, p), lib.adaf_resnet50_workspace_bytes(trunk._net, n, p), shift_place=place)


def main():
    lib = _lib.load_library()
    for q, args, v in host_sizes(lib):
        emit(q, args, v)
    if "--host" not in sys.argv[1:]:
        device_sizes(lib)


if __name__ == "__main__":
    main()
