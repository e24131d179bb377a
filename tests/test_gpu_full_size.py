"""Parameter sets at the reference's FULL size on the MI355X (pytest -m gpu), through the checks of tests/full_size_checks.py: MK32 (32 parties,
n = 620, N = 2048: the three-part-digit pair kernel behind the MK32 ... MK128 numbers) as gates and as a lookup table, KMS2 at n = 560, CCS4.
Every check returns its record; the asserts are on the words compared with the CPU oracle and on the decryptions.  The key switches
(thfhe_keyswitch.h) run ks_staged_kernel from 192 samples on (the 512 MK32 gates) and ks_plain_kernel below."""
import pytest

import full_size_checks as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk32(O):
    keys = F.mk_keys("MK32")   # device key generation, 1.3 GB of key coefficients
    yield keys
    keys[2].close()


def test_mk32_gates_full_size(mk32):
    # 512 NANDs = 256 workgroups of the pair kernel; gates 0 and 1 share the first workgroup, 511 is the last one's second gate
    rec = F.mk_check("MK32", 512, [0, 1, 511], keys=mk32)
    assert rec["kernel"] == "mk_blind_rotate_pair2k_kernel<3>"
    assert rec["all_decrypt_correct"]
    assert rec["words_equal_to_oracle"] and rec["words_compared"] == 3 * (32 * 620 + 1)


def test_mk32_lut_full_size(mk32):
    # 3 samples on the pair kernel (threshold 0): sample 2 is the lone job of the last workgroup
    rec = F.mk_lut_check("MK32", 3, 2, (0, 2), mk32, pair_threshold=0)
    assert rec["kernel"] == "mk_blind_rotate_pair2k_kernel<3>"
    assert rec["wo_keyswitch_equal_to_reference"]
    assert rec["keyswitched_equal_to_reference"]
    assert rec["words_compared"] == 2 * 2 * (2048 + 1 + 32 * 620 + 1)


def test_kms2_full_size():
    # the reference's KMS2 set at n = 560 (the other KMS tests stop at n = 96): 8 gates and 8 fast_boot gates word for word
    rec = F.kms2_check(gates=8, batch=256)
    assert rec["words_equal_to_oracle"] and rec["fast_boot_words_equal_to_oracle"]
    assert rec["all_decrypt_correct"] and rec["fast_boot_all_decrypt_correct"]
    assert rec["words_compared"] == 2 * 8 * (2 * 560 + 1)


def test_ccs4_full_size():
    rec = F.ccs_oracle_check("CCS4", 128, 4)
    assert rec["words_equal_to_oracle"] and rec["words_compared"] == 4 * (4 * 560 + 1)
    assert rec["all_decrypt_correct"]
