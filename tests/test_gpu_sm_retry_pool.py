"""The sm_retry option of the Python pools (BlsGpuVerifier,
BlsGpuSingleThreadVerifier): off by default, every context switched when on,
and the sm_retry_subs / sm_retry_leaves / sm_retry_pairs metrics fed from
bgv_sm_retry_stats.  One call of 64 sets with one bad signature."""
import asyncio

import numpy as np
import pytest

from tests.test_gpu_same_message import msg_of, sign

pytestmark = pytest.mark.gpu

SEED = 0x504F4F4C
SPLIT = {"sm_retry_subs": 8, "sm_retry_leaves": 8, "sm_retry_pairs": 32}
PER_SET = {"sm_retry_subs": 0, "sm_retry_leaves": 64, "sm_retry_pairs": 128}


def test_pool_option_and_metrics():
    from lodestar_amd import verifier as V

    async def main():
        m = msg_of(7000)
        for on, want in ((False, PER_SET), (True, SPLIT)):
            v = V.BlsGpuVerifier(devices=(0,), contexts_per_device=1, sm_retry=on) if on else V.BlsGpuVerifier(
                devices=(0,), contexts_per_device=1)
            try:
                assert v.sm_retry is on
                for d in v._contexts():
                    d.gen_keys(0, 64, SEED)
                sigs = sign(v.devices[0], np.arange(64, dtype=np.uint32), np.stack([np.frombuffer(m, np.uint8)] * 64))
                sets = [(V.PublicKey(index=i), sigs[i, :96].tobytes()) for i in range(64)]
                sets[29] = (sets[29][0], sets[30][1])  # another validator's signature
                expected = [i != 29 for i in range(64)]
                assert {k: v.metrics[k] for k in want} == dict.fromkeys(want, 0)
                assert await v.verify_signature_sets_same_message(sets, m) == expected
                assert {k: v.metrics[k] for k in want} == want
                assert v.metrics["same_message_retries"] == 1
                # every context of the pool carries the switch, the priority context too
                for d in v._contexts():
                    d.gen_keys(0, 64, SEED)
                    ok, _ = d.verify_same_message(V.encode_same_message([(m, sets)], None))
                    assert ok.tolist() == expected and d.sm_retry_stats()["mode"] == int(on)
                s = V.BlsGpuSingleThreadVerifier(0, sm_retry=on)
                try:
                    s.device.gen_keys(0, 64, SEED)
                    assert await s.verify_signature_sets_same_message(sets, m) == expected
                    assert s.device.sm_retry_stats()["mode"] == int(on)
                    assert s.device.sm_retry_stats()["subs"] == want["sm_retry_subs"]
                finally:
                    await s.close()
            finally:
                await v.close()

    asyncio.run(main())
