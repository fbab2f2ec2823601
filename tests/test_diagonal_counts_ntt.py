"""diagonal.dense_path_counts(..., ntt_weights=True): the limb transforms of the two dense paths when the weight plaintexts are resident in NTT form
(hewrapper.NTT_WEIGHTS), written out by hand for the five layers of DESIGN §6g's table.

A key switch is digits k forward + 2 k inverse transforms on either path.  Default path: 2 k forward for the ciphertext, per row 2 k inverse of the row product
(its 2 k forward transforms of the row plaintext are gone) and 7 k of the mask product.  Diagonal path: 2 k forward per rotated input and 2 k inverse per group (the
2 k forward per diagonal are gone).  The structure of every layer - key switches, diagonals, baby steps, groups - is that of the table and does not depend on the flag."""
import pytest

from cryptonets_amd import diagonal

# (R, Dim, N, k, digits): default key switches; diagonal key switches, rotated inputs, groups; diagonals
LAYERS = [
    ((5488, 16268, 16384, 8, 8), 76832, (254, 128, 128), 16384),
    ((2608, 11952, 16384, 7, 7), 36512, (241, 128, 115), 14559),
    ((10, 5488, 16384, 8, 8), 140, (149, 64, 87), 5497),
    ((3, 1000, 1024, 3, 6), 30, (62, 32, 32), 1002),
    ((37, 700, 1024, 3, 6), 370, (54, 32, 24), 736),
]
# the totals, by hand: key switches x (digits k + 2 k) + the plaintext side
BY_HAND = [
    (76832 * 80 + 16 + 5488 * 16 + 5488 * 56, 254 * 80 + 128 * 16 + 128 * 16),        # 6 541 712, 24 416
    (36512 * 63 + 14 + 2608 * 14 + 2608 * 49, 241 * 63 + 128 * 14 + 115 * 14),        # 2 464 574, 18 585
    (140 * 80 + 16 + 10 * 16 + 10 * 56, 149 * 80 + 64 * 16 + 87 * 16),                # 11 936, 14 336
    (30 * 24 + 6 + 3 * 6 + 3 * 21, 62 * 24 + 32 * 6 + 32 * 6),                        # 807, 1 872
    (370 * 24 + 6 + 37 * 6 + 37 * 21, 54 * 24 + 32 * 6 + 24 * 6),                     # 9 885, 1 632
]
TOTALS = [(6541712, 24416), (2464574, 18585), (11936, 14336), (807, 1872), (9885, 1632)]


@pytest.mark.parametrize("layer,by_hand,totals", list(zip(LAYERS, BY_HAND, TOTALS)), ids=["cifar", "large", "10x5488", "3x1000", "37x700"])
def test_counts_without_the_plaintext_transforms(layer, by_hand, totals):
    (R, Dim, n, k, digits), d_ks, (g_ks, babies, groups), diagonals = layer
    assert by_hand == totals
    c = diagonal.dense_path_counts(R, Dim, n, k, digits, ntt_weights=True)
    assert (c["default_key_switches"], c["diagonal_key_switches"], c["babies"], c["groups"], c["diagonals"]) == (d_ks, g_ks, babies, groups, diagonals)
    assert (c["default"], c["diagonal"]) == totals
    assert c["choice"] == ("diagonal" if totals[1] < totals[0] else "default")
    # against the coefficient form: 2 k per row and 2 k per diagonal less, nothing else
    p = diagonal.dense_path_counts(R, Dim, n, k, digits)
    assert p["default"] - c["default"] == R * 2 * k and p["diagonal"] - c["diagonal"] == diagonals * 2 * k
    assert p == diagonal.dense_path_counts(R, Dim, n, k, digits, ntt_weights=False)


def test_the_choices_of_the_table_do_not_change():
    assert [diagonal.dense_path_counts(*l[0], ntt_weights=True)["choice"] for l in LAYERS] == ["diagonal", "diagonal", "default", "default", "diagonal"]
