"""GPU: true-length masking of the attention kernels through voice plans — ragged batches whose items end far below the bucket, at the
edges of the 16-key tiles and of the 32-key prefetch chunks (1, 16, 17, 33, 65, 97, 129) and just below it. One frame per id (F = T).

The walker of tests/front_ref.py checks every front step of every item, teacher-forced from the GPU's own buffers; steps of kind
`rel_attention` are held to the rule without the floor, |Δ| ≤ OP_TOL · ‖ref‖∞, in addition (front_ref.verify(att_floorless=True),
tests/att_ref.py says why). z is compared with the C oracle for the items of at most 129 ids; the long items are covered step by step.

Routes on 256 CUs (blocks = ⌈Tb/16⌉ · heads · items against the CU count, csrc/attention.hip):
  bucket 1040, 7 items     register-fragment kernel, 16 query rows per block       (d 96 medium, d 48 x_low)
  bucket 2064, 4 items     register-fragment kernel, 8 query rows per block
  bucket 656, 5 items      staged-tile kernel UNSPLIT over six key tiles: 410 blocks leave no room for parts
  bucket 336, 2 items      staged-tile kernel key-split in THREE parts + merge (84 blocks): an item of 5 ids has two parts without a
                           key (the kernel and the merge skip them by the same tile rule), one of 129 ids has one"""
import numpy as np
import pytest

import att_ref as ar
import front_ref as fr
import piper_hip as ph
from test_gpu_front_exact import run_and_verify

pytestmark = pytest.mark.gpu

BATCHES = {
    1040: (1030, 1, 17, 33, 65, 129, 1025),
    2064: (2050, 16, 97, 1040),
    656: (650, 5, 129, 300, 513),
}
THREE_PARTS = ((330, 5), (330, 129))


@pytest.fixture(scope="module")
def rt_of(backend):
    made = {}

    def get(quality):
        if quality not in made:
            cfg = ph.voice_config(quality)
            blob = ph.synthetic_blob(cfg, 1234)
            made[quality] = (ph.HipRuntime(backend, cfg, blob), cfg, blob)
        return made[quality]
    yield get
    for rt, _, _ in made.values():
        rt.close()


def ragged(rt_of, quality, Ts, bucket, slot):
    rt, cfg, blob = rt_of(quality)
    utts = [fr.utterance(cfg, T, T, 5000 + 3 * T + b) for b, T in enumerate(Ts)]
    label = f"{quality} lengths {'/'.join(map(str, Ts))}"
    _, rows, steps = run_and_verify(rt, blob, slot, utts, label, z_max_ids=129, att_floorless=True)
    assert rt.plan_info(slot)["bucket_t"] == bucket
    att = [r for r in rows if r[3] == "rel_attention"]
    assert len(att) == cfg.n_layers * len(Ts) and all("floorless" in r[4] and r[4]["ok"] for r in att)
    assert {r[2] for r in rows} == set(range(len(Ts)))
    return cfg, att


@pytest.mark.parametrize("quality", ["medium", "x_low"])
@pytest.mark.parametrize("bucket", [1040, 2064])
def test_register_fragment_kernels_ragged(quality, bucket, rt_of):
    cfg, _ = ragged(rt_of, quality, BATCHES[bucket], bucket, 0)
    d = cfg.hidden // cfg.n_heads
    assert ar.route_of(d, bucket, cfg.window, cfg.n_heads, len(BATCHES[bucket]))[0] == ("mfma16" if bucket == 1040 else "mfma8")


def test_staged_tile_kernel_ragged_over_six_key_tiles(rt_of):
    cfg, _ = ragged(rt_of, "medium", BATCHES[656], 656, 1)
    assert ar.route_of(96, 656, cfg.window, cfg.n_heads, 5) == ("lds", 1)  # (a single utterance of 650 ids runs in three parts)


@pytest.mark.parametrize("Ts", THREE_PARTS, ids=lambda t: "/".join(map(str, t)))
def test_three_key_parts_with_parts_past_the_length(Ts, rt_of):
    cfg, _ = ragged(rt_of, "medium", Ts, 336, 2)
    assert ar.route_of(96, 336, cfg.window, cfg.n_heads, 2) == ("lds_split", 3)
    assert [min(3, -(-T // 128)) for T in Ts] == [3, 1 if Ts[1] == 5 else 2]  # key parts that hold a key of each item
