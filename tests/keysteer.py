"""Keys with a chosen 64-bit hash, for the string-key table's tests (plain Python integers, no GPU, no library).

mix64 / hash_key restate throttlecrab_amd/csrc/key_table.hpp:111-153 (mix64, load_tail, hash_key).  mix64 is the Murmur3
finaliser: three xor-shifts by 33 (each its own inverse: 2 * 33 >= 64) and two multiplications by odd constants (invertible
mod 2^64), so it is a bijection on u64.  hash_key chains it over the key's 8-byte words, hence any key with at least one FULL
word can be given any hash: run the chain forwards up to that word, backwards from the wanted hash down to it, and solve for
the word.  tests/test_key_hash_model.py holds this restatement against the library (tc_route_keys_host).

Keys of one length <= 8 bytes cannot collide: their hash is mix64 of ONE word that holds the whole key, and mix64 is
injective.  Twins therefore need at least 9 bytes (a full word to steer and something else to differ in).
"""
M64 = (1 << 64) - 1
C = 0x9e3779b97f4a7c15
M1, M2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
M1_INV, M2_INV = pow(M1, -1, 1 << 64), pow(M2, -1, 1 << 64)
ROUTE_SALT = 0xa5a5a5a5a5a5a5a5  # route.hip:187-195: owner = mix64(hash_key(key) ^ salt) % world
RT_VALID = 1 << 63               # key_table.hpp: a retired record's tag is hash | RT_VALID, its home (hash >> 17) & (RETIRED_CAP - 1)
RETIRED_CAP = 65536


def mix64(x):
    x ^= x >> 33
    x = x * M1 & M64
    x ^= x >> 33
    x = x * M2 & M64
    x ^= x >> 33
    return x


def inv_mix64(x):
    x ^= x >> 33
    x = x * M2_INV & M64
    x ^= x >> 33
    x = x * M1_INV & M64
    x ^= x >> 33
    return x


def _tail(key, at):
    """what the chain mixes in for the 1..7 bytes behind the last full word: load_tail() ^ count << 56"""
    r = len(key) - at
    return int.from_bytes(key[at:], "little") ^ (r << 56)


def hash_key(key: bytes):
    n = len(key)
    h = C ^ n
    i = 0
    while i + 8 <= n:
        h = (mix64(h ^ int.from_bytes(key[i:i + 8], "little")) + C) & M64
        i += 8
    if i < n:
        h = mix64(h ^ _tail(key, i))
    return mix64(h)


def owner(key: bytes, world: int):
    return mix64(hash_key(key) ^ ROUTE_SALT) % world


def table_size(capacity: int):
    """entries of an engine's key table: the smallest power of two >= 2 * capacity (engine.hip:322-323)"""
    nb = 1
    while nb < 2 * capacity:
        nb <<= 1
    return nb


def steer(key: bytes, target_hash: int, word: int):
    """`key` with its full 8-byte word number `word` replaced so that hash_key(result) == target_hash (same length)"""
    n = len(key)
    if not (n >= 8 and 0 <= word < n // 8):
        raise ValueError(f"word {word} is not a full 8-byte word of a {n}-byte key")
    h = C ^ n                                    # forwards: the state in front of the steered word
    for j in range(word):
        h = (mix64(h ^ int.from_bytes(key[8 * j:8 * j + 8], "little")) + C) & M64
    s = inv_mix64(target_hash)                   # backwards: the state behind it
    if n % 8:
        s = inv_mix64(s) ^ _tail(key, n - n % 8)
    for j in range(n // 8 - 1, word, -1):
        s = inv_mix64((s - C) & M64) ^ int.from_bytes(key[8 * j:8 * j + 8], "little")
    w = inv_mix64((s - C) & M64) ^ h
    out = key[:8 * word] + w.to_bytes(8, "little") + key[8 * word + 8:]
    assert hash_key(out) == target_hash and len(out) == n
    return out


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype="uint8").tobytes()


def steer_word(length: int):
    """the word the builders steer: word 2 where the key has one that holds neither word 1 nor the last byte, else word 0"""
    return 2 if length >= 25 else 0


def twins(length: int, m: int, rng, target=None):
    """m distinct keys of `length` >= 9 bytes with one hash.  Member 1 differs from member 0 only in the steered word and the
    last byte, member 2 from member 0 only in the steered word and byte 8 (word 1); the others are unrelated bytes."""
    if length < 9:
        raise ValueError("keys of one length <= 8 bytes cannot collide (one injective mix64 of one word)")
    sw = steer_word(length)
    target = int(rng.integers(0, 1 << 64, dtype="uint64")) if target is None else target
    base = bytearray(_bytes(rng, length))
    out = []
    for j in range(m):
        k = bytearray(base) if j < 3 else bytearray(_bytes(rng, length))
        if j == 1:
            k[-1] ^= 0x01
        if j == 2:
            k[8] ^= 0x80
        out.append(steer(bytes(k), target, sw))
    assert len(set(out)) == m
    return out


def cross_length(lengths, rng, target=None):
    """one key per length (ascending, all > 16) with one hash; each is a byte prefix of the next.  The steered word of a key
    lies wholly behind the end of the key before it, so steering never touches the shared prefix."""
    target = int(rng.integers(0, 1 << 64, dtype="uint64")) if target is None else target
    out, prev = [], b""
    for n in lengths:
        w = (len(prev) + 7) // 8
        if not (n > 16 and n > len(prev) and 8 * w + 8 <= n):
            raise ValueError(f"no full word of a {n}-byte key behind {len(prev)} shared bytes")
        prev = steer(prev + _bytes(rng, n - len(prev)), target, w)
        out.append(prev)
    return out


def home_hash(pos: int, nb: int, rng, tag=None):
    """a hash whose home in a table of nb entries (h & (nb - 1)) is `pos` and, if asked, whose tag (bits 40..63) is `tag`"""
    assert nb & (nb - 1) == 0 and 0 <= pos < nb <= 1 << 40
    h = int(rng.integers(0, 1 << 64, dtype="uint64"))
    h = (h & ~(nb - 1) & M64) | pos
    if tag is not None:
        h = (h & ((1 << 40) - 1)) | (tag << 40)
    return h


def at_home(pos: int, nb: int, rng, length: int = 24, tag=None):
    """a random key of `length` >= 8 bytes whose home is `pos` (and whose tag is `tag`)"""
    return steer(_bytes(rng, length), home_hash(pos, nb, rng, tag), steer_word(length))


def owned_by(dest: int, world: int, rng, length: int):
    """a random key of `length` bytes that tc_route_keys gives to destination `dest`: targets are drawn until
    mix64(t ^ salt) % world fits, then the key is steered there.  A key without a full word cannot be steered: keys are drawn
    instead, and None comes back where none fits (the empty key has one owner)."""
    if length < 8:
        for _ in range(64 * world if length else 1):
            k = _bytes(rng, length)
            if owner(k, world) == dest:
                return k
        return None
    import numpy as np
    while True:  # (a handful of targets per draw, mixed by numpy in wrapping uint64 arithmetic: 3 000-key arenas stay quick)
        t = rng.integers(0, 1 << 64, 4 * world, dtype=np.uint64)
        x = t ^ np.uint64(ROUTE_SALT)
        for m in (M1, M2):
            x ^= x >> np.uint64(33)
            x *= np.uint64(m)
        x ^= x >> np.uint64(33)
        fits = t[x % np.uint64(world) == np.uint64(dest)]
        if len(fits):
            assert mix64(int(fits[0]) ^ ROUTE_SALT) % world == dest
            return steer(_bytes(rng, length), int(fits[0]), int(rng.integers(0, length // 8)))
