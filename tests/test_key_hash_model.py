"""tests/keysteer.py restates the key table's hash in Python integers; the GPU tests of colliding keys (test_gpu_key_collisions.py)
rest on it.  Here the restatement is held against the library -- through tc_route_keys_host, the one host call that shows a
function of the hash -- and the builders against what they promise."""
import numpy as np

from tests import keysteer as ks


def _keys():
    rng = np.random.default_rng(1)
    lens = [j % 131 for j in range(1965)] + [300] * 35
    keys = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    keys += [b"", b"\0" * 8, b"\xff" * 16, b"\0" * 17, b"\xff" * 7, b"user:123", b"key_1234567"]
    return keys


def test_hash_key_equals_the_librarys_hash():
    """owner = mix64(hash_key(key) ^ salt) % world (route.hip:187-195) for every world 1..64.  lcm(1..64) > 2^64, so by the
    Chinese remainder theorem the 64 residues fix the mixed value, and mix64 being a bijection they fix the hash itself."""
    from oracle import oracle as O
    from throttlecrab_amd import sharded
    keys = _keys()
    kb, ko = O.pack_keys(keys)
    mixed = [ks.mix64(ks.hash_key(k) ^ ks.ROUTE_SALT) for k in keys]
    assert int(np.lcm.reduce(np.arange(1, 65, dtype=object))) > 1 << 64
    for world in range(1, 65):
        got = sharded.route_keys(kb, ko, world)
        assert got.tolist() == [m % world for m in mixed], world
        assert got[:50].tolist() == [ks.owner(k, world) for k in keys[:50]]


def test_inv_mix64_inverts_mix64():
    rng = np.random.default_rng(2)
    xs = [0, 1, ks.M64, 1 << 63, 1 << 33, (1 << 33) - 1] + [int(x) for x in rng.integers(0, 1 << 64, 5000, dtype=np.uint64)]
    for x in xs:
        assert ks.inv_mix64(ks.mix64(x)) == x and ks.mix64(ks.inv_mix64(x)) == x


def test_steered_keys_hit_their_target():
    rng = np.random.default_rng(3)
    for n in list(range(8, 131)) + [200, 300]:
        key = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for word in range(n // 8):  # every admissible steering word
            target = int(rng.integers(0, 1 << 64, dtype=np.uint64))
            out = ks.steer(key, target, word)
            assert ks.hash_key(out) == target and len(out) == n
            assert out[:8 * word] == key[:8 * word] and out[8 * word + 8:] == key[8 * word + 8:]
    for bad in ((b"1234567", 0), (b"123456789", 1), (b"12345678", -1)):
        try:
            ks.steer(bad[0], 0, bad[1])
        except ValueError:
            continue
        raise AssertionError(bad)


def test_twins_are_distinct_and_differ_where_they_say():
    rng = np.random.default_rng(4)
    for n in (9, 12, 16, 17, 24, 25, 40, 64, 65, 112, 113, 200):
        g = ks.twins(n, 4, rng)
        assert len(set(g)) == 4 and len({ks.hash_key(k) for k in g}) == 1 and {len(k) for k in g} == {n}
        sw = ks.steer_word(n)
        diff = lambda a, b: {i for i in range(n) if a[i] != b[i]} - set(range(8 * sw, 8 * sw + 8))
        assert diff(g[0], g[1]) == {n - 1} and diff(g[0], g[2]) == {8}
    try:
        ks.twins(8, 2, rng)
    except ValueError:
        pass
    else:
        raise AssertionError("twins of 8 bytes")


def test_cross_length_keys_share_a_prefix_and_a_hash():
    rng = np.random.default_rng(5)
    for lens in ((24, 32, 72, 120, 200), (17, 64, 72), (112, 120)):
        g = ks.cross_length(lens, rng)
        assert [len(k) for k in g] == list(lens) and len({ks.hash_key(k) for k in g}) == 1
        assert all(b.startswith(a) for a, b in zip(g, g[1:]))


def test_homes_tags_and_owners_are_as_chosen():
    rng = np.random.default_rng(6)
    assert [ks.table_size(c) for c in (1, 1024, 1025, 2048, 4096)] == [2, 2048, 4096, 4096, 8192]
    for nb in (2048, 8192):
        for n in (8, 9, 16, 17, 64, 65, 113, 200):
            h = ks.hash_key(ks.at_home(nb - 3, nb, rng, n, tag=0xABCDEF))
            assert h & (nb - 1) == nb - 3 and h >> 40 == 0xABCDEF
            assert ks.hash_key(ks.at_home(5, nb, rng, n)) & (nb - 1) == 5
    for world in (3, 64):
        for n in (1, 7, 8, 33, 300):
            k = ks.owned_by(world - 1, world, rng, n)
            assert k is None and n < 8 or len(k) == n and ks.owner(k, world) == world - 1
    assert ks.owned_by((ks.owner(b"", 3) + 1) % 3, 3, rng, 0) is None and ks.owned_by(ks.owner(b"", 3), 3, rng, 0) == b""
