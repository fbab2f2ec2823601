"""Wire formats: SEAL 3.2 object streams, the wrapper's text + base64 framing, the zip key container.

Two layers, as in the reference:

* wrapper framing - exact, taken from the reference source: `AtomicSealBfvEncryptedVector.Write/Read`
  (AtomicSealBfvVector.cs:1273-1345), `EncryptedSealBfvVector.Write/Read` (EncryptedSealBfvVector.cs:414-439),
  `EncryptedSealBfvMatrix.Write/Read` (EncryptedSealBfvMatrix.cs:182-208), `AtomicSealBfvEncryptedEnvironment.SaveToStream /
  LoadFromStream` (AtomicSealBfvVector.cs:93-130: parameters, public key, relin keys, Galois keys, secret key - an EMPTY secret
  key when saved without private keys) and the zip of `environmentNNN` entries, stored uncompressed
  (EncryptedSealBfvVector.cs:104-134).

* SEAL object streams - the payload inside that framing is produced by SEAL 3.2's own `Save` methods, which are NOT in the
  reference repository (SEALNet 3.2.0 is an un-vendored NuGet dependency, `HE Wrapper/packages.config:6`).  The layouts below
  restate the published SEAL 3.2 `save()` members (all little-endian, no compression in 3.2):

      EncryptionParameters  u8 scheme (1 = BFV) | u64 poly_modulus_degree | u64 coeff_mod_count | u64 q[...] | u64 plain_modulus
                            | f64 noise_standard_deviation
      parms_id              SHA3-256 over the u64 words [scheme, N, q..., t, bits(noise_standard_deviation)] -> 4 x u64
      IntArray<u64>         u64 count | count x u64
      Plaintext             parms_id | f64 scale | IntArray coefficients      (BFV plaintexts carry the all-zero parms_id)
      Ciphertext            parms_id | u8 is_ntt_form | u64 size | u64 poly_modulus_degree | u64 coeff_mod_count | f64 scale
                            | IntArray data, laid out [poly][limb][coefficient]
      PublicKey             the Ciphertext (c0, c1) in NTT form;   SecretKey: a Plaintext of k*N words (NTT form, key parms_id)
      RelinKeys/GaloisKeys  parms_id | i32 decomposition_bit_count | u64 dim1 | dim1 x ( u64 dim2 | dim2 x Ciphertext )
                            RelinKeys: dim1 = 1 (key for s^2), dim2 = number of (limb, digit) pairs, each a size-2 NTT-form
                            ciphertext - the layout libcnhip keeps in HBM (include/cnhip.h).  GaloisKeys: dim1 = N, entry
                            (galois_elt - 1) / 2 holds that element's digits, absent elements have dim2 = 0.

* compact batches - this library's own framing of seeded symmetric ciphertexts (c0 words and a public seed; `save_compact_batch` /
  `load_compact_batch` below).  NOT a SEAL 3.2 stream.
* packed rows and packed batches - the same batches with every residue in bit_length(q_j) bits (`pack_rows`, `save_packed_batch` below).

  PARITY UNPINNED: no SEAL binary or SEAL-written file exists in this environment or in the reference repository, so byte
  compatibility with real SEAL 3.2 streams is restated, not tested.  What the tests pin is self-consistency (round trips of
  every object, rejection of foreign parameters / truncated streams) and the wrapper framing against the reference source.
"""
import base64
import hashlib
import io
import struct
import zipfile

import numpy as np

SCHEME_BFV = 1
DEFAULT_NOISE_STANDARD_DEVIATION = 3.20          # SEAL 3.2 util::global_variables::default_noise_standard_deviation
PARMS_ID_ZERO = b"\0" * 32


class BadStream(Exception):
    """the reference throws Exception("Bad stream format.")"""


# ------------------------------------------------------------------------------------------------ primitives
def _rd(f, nbytes):
    b = f.read(nbytes)
    if len(b) != nbytes:
        raise BadStream("Bad stream format. (truncated)")
    return b


def _w_u64(f, v):
    f.write(struct.pack("<Q", int(v)))


def _r_u64(f):
    return struct.unpack("<Q", _rd(f, 8))[0]


def _w_array(f, words):
    a = np.ascontiguousarray(words, dtype="<u8").reshape(-1)
    _w_u64(f, a.size)
    f.write(a.tobytes())


def _r_array(f, limit=1 << 31):
    count = _r_u64(f)
    if count > limit:
        raise BadStream("Bad stream format. (array of %d words)" % count)
    return np.frombuffer(_rd(f, 8 * count), dtype="<u8").astype(np.uint64)


class Parameters:
    """EncryptionParameters of one environment (scheme BFV)."""

    def __init__(self, n, q, t, noise_standard_deviation=DEFAULT_NOISE_STANDARD_DEVIATION):
        self.n, self.q, self.t, self.sigma = int(n), [int(x) for x in q], int(t), float(noise_standard_deviation)

    @property
    def k(self):
        return len(self.q)

    def parms_id(self):
        words = [SCHEME_BFV, self.n, *self.q, self.t, struct.unpack("<Q", struct.pack("<d", self.sigma))[0]]
        return hashlib.sha3_256(struct.pack("<%dQ" % len(words), *words)).digest()

    def save(self, f):
        f.write(struct.pack("<B", SCHEME_BFV))
        _w_u64(f, self.n)
        _w_u64(f, self.k)
        for q in self.q:
            _w_u64(f, q)
        _w_u64(f, self.t)
        f.write(struct.pack("<d", self.sigma))

    @classmethod
    def load(cls, f):
        scheme = struct.unpack("<B", _rd(f, 1))[0]
        if scheme != SCHEME_BFV:
            raise BadStream("unsupported scheme %d (BFV expected)" % scheme)
        n, k = _r_u64(f), _r_u64(f)
        if n < 2 or n & (n - 1) or n > 32768 or not 1 <= k <= 64:
            raise BadStream("Bad stream format. (parameters)")
        q = [_r_u64(f) for _ in range(k)]
        t = _r_u64(f)
        sigma = struct.unpack("<d", _rd(f, 8))[0]
        return cls(n, q, t, sigma)

    def __eq__(self, o):
        return (self.n, self.q, self.t, self.sigma) == (o.n, o.q, o.t, o.sigma)

    def level(self, limbs):
        """the parameters of a level of this chain: q[:limbs] (SEAL 3.2 has no special prime - every prefix of q is a level), same N, t, sigma"""
        if not 1 <= limbs <= self.k:
            raise ValueError("a level keeps 1 .. %d coefficient moduli (got %d)" % (self.k, limbs))
        return Parameters(self.n, self.q[:limbs], self.t, self.sigma)

    def chain(self):
        """{parms_id: limbs} of every level of the chain, the first (all of q) included"""
        return {self.level(l).parms_id(): l for l in range(1, self.k + 1)}


# ------------------------------------------------------------------------------------------------ SEAL objects
def save_plaintext(f, coeffs, parms_id=PARMS_ID_ZERO, scale=1.0):
    f.write(parms_id)
    f.write(struct.pack("<d", scale))
    _w_array(f, coeffs)


def load_plaintext(f, parms=None, expect_parms_id=PARMS_ID_ZERO):
    pid = _rd(f, 32)
    if expect_parms_id is not None and pid != expect_parms_id:
        raise BadStream("plaintext is not valid for the encryption parameters")
    struct.unpack("<d", _rd(f, 8))
    data = _r_array(f)
    if parms is not None and expect_parms_id == PARMS_ID_ZERO and (data.size > parms.n or (data.size and int(data.max()) >= parms.t)):
        raise BadStream("plaintext is not valid for the encryption parameters")
    return data


def save_ciphertext(f, words, parms, size=2, is_ntt_form=False, scale=1.0):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if w.size != size * parms.k * parms.n:
        raise ValueError("ciphertext has %d words, expected %d" % (w.size, size * parms.k * parms.n))
    f.write(parms.parms_id())
    f.write(struct.pack("<B", 1 if is_ntt_form else 0))
    _w_u64(f, size)
    _w_u64(f, parms.n)
    _w_u64(f, parms.k)
    f.write(struct.pack("<d", scale))
    _w_array(f, w)


def load_ciphertext(f, parms, want_ntt_form=None):
    """-> (words, size); Ciphertext.Load(context, stream) validity checks: parms_id of THIS context, consistent sizes,
    residues below their moduli"""
    if _rd(f, 32) != parms.parms_id():
        raise BadStream("ciphertext is not valid for the encryption parameters")
    ntt = struct.unpack("<B", _rd(f, 1))[0]
    size, n, k = _r_u64(f), _r_u64(f), _r_u64(f)
    struct.unpack("<d", _rd(f, 8))
    if ntt > 1 or n != parms.n or k != parms.k or not 2 <= size <= 16 or (want_ntt_form is not None and bool(ntt) != want_ntt_form):
        raise BadStream("ciphertext is not valid for the encryption parameters")
    data = _r_array(f)
    if data.size != size * k * n:
        raise BadStream("Bad stream format. (ciphertext data)")
    limbs = data.reshape(size, k, n)
    for j, q in enumerate(parms.q):
        if int(limbs[:, j].max()) >= q:
            raise BadStream("ciphertext is not valid for the encryption parameters")
    return data, int(size)


def load_ciphertext_any_level(f, parms, want_ntt_form=None):
    """-> (words, size, limbs): Ciphertext.Load + is_valid_for of SEAL 3.2 for a context with a modulus-switching chain - the parms_id may be
    that of any level of `parms` (q[:limbs], 1 <= limbs <= k); sizes and residues are checked against that level's moduli.
    load_ciphertext accepts the first level only."""
    pid = _rd(f, 32)
    limbs = parms.chain().get(pid)
    if limbs is None:
        raise BadStream("ciphertext is not valid for the encryption parameters")
    data, size = load_ciphertext(_Prefixed(pid, f), parms.level(limbs), want_ntt_form)
    return data, size, limbs


# ------------------------------------------------------------------------------------------------ compact batches of seeded ciphertexts
# NOT a SEAL 3.2 stream (SEAL ships seeded ciphertexts from 3.4 on, with another generator and another layout): this library's own framing of a batch
# of fresh secret-key encryptions whose c1 is regenerated from a public seed (include/cnhip.h: cn_encrypt_symmetric, cn_ct_upload_compact).
#     8 B magic "CNHIPSC1" | u32 version (1) | 32 B public seed | u64 nonce | u64 first item | u64 count | 32 B parms_id of the level
#     | IntArray of count * k * N words: the c0 polynomials, [ciphertext][limb][coefficient]                       (all little-endian)
COMPACT_MAGIC = b"CNHIPSC1"
COMPACT_VERSION = 1


class CompactDescriptor:
    """what turns c0 words back into ciphertexts: the public seed (32 bytes), the nonce, the first item, the count and the parms_id of the level"""

    def __init__(self, a_seed, a_nonce, a_item0, count, parms_id):
        self.a_seed, self.a_nonce, self.a_item0, self.count, self.parms_id = bytes(a_seed), int(a_nonce), int(a_item0), int(count), bytes(parms_id)
        if len(self.a_seed) != 32 or len(self.parms_id) != 32:
            raise ValueError("the public seed and the parms_id have 32 bytes")

    def __eq__(self, o):
        return (self.a_seed, self.a_nonce, self.a_item0, self.count, self.parms_id) == (o.a_seed, o.a_nonce, o.a_item0, o.count, o.parms_id)


def save_compact_batch(f, c0, desc):
    c0 = np.ascontiguousarray(c0, dtype=np.uint64)
    if c0.ndim != 2 or c0.shape[0] != desc.count:
        raise ValueError("c0 words of shape %s do not belong to a descriptor of %d ciphertexts" % (c0.shape, desc.count))
    f.write(COMPACT_MAGIC)
    f.write(struct.pack("<I", COMPACT_VERSION))
    f.write(desc.a_seed)
    _w_u64(f, desc.a_nonce)
    _w_u64(f, desc.a_item0)
    _w_u64(f, desc.count)
    f.write(desc.parms_id)
    _w_array(f, c0)


def load_compact_batch(f, parms):
    """(c0 words [count, limbs * N], descriptor, limbs); `parms`: the Parameters of the chain's first level - a batch of any of its levels loads"""
    if _rd(f, 8) != COMPACT_MAGIC:
        raise BadStream("Bad stream format. (not a compact batch)")
    version = struct.unpack("<I", _rd(f, 4))[0]
    if version != COMPACT_VERSION:
        raise BadStream("compact batch of version %d (this library reads %d)" % (version, COMPACT_VERSION))
    a_seed = _rd(f, 32)
    a_nonce, a_item0, count = _r_u64(f), _r_u64(f), _r_u64(f)
    pid = _rd(f, 32)
    limbs = parms.chain().get(pid)
    if limbs is None:
        raise BadStream("the compact batch belongs to other encryption parameters")
    if (a_item0 + count) >> 40:
        raise BadStream("Bad stream format. (items)")
    words = _r_array(f)
    if words.size != count * limbs * parms.n:
        raise BadStream("Bad stream format. (%d words for %d ciphertexts of %d limbs)" % (words.size, count, limbs))
    return words.reshape(count, limbs * parms.n), CompactDescriptor(a_seed, a_nonce, a_item0, count, pid), limbs


# ------------------------------------------------------------------------------------------------ packed rows and packed batches
# The library's own wire form without padding bits (include/cnhip.h: cn_packed_words, cn_ct_upload_packed; NOT a SEAL stream): the residues of one
# polynomial limb in bits = bit_length(q_j) bits each.  The row is the integer sum_i v_i 2^(i bits), cut into little-endian 64-bit words: coefficient i
# occupies bits [i bits, (i + 1) bits) of the row, bit p of the row is bit p % 64 of word p / 64.  n * bits is a multiple of 64 (n is a multiple of 64).
def pack_rows(words, bits):
    """uint64 [..., n] residues below 2^bits (2 <= bits <= 60) -> uint64 [..., n * bits / 64] packed rows"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    bits, n = int(bits), w.shape[-1]
    if not 2 <= bits <= 60 or (n * bits) % 64:
        raise ValueError("pack_rows: 2 <= bits <= 60 and n * bits a multiple of 64 (got bits %d, n %d)" % (bits, n))
    if w.size and int(w.max()) >> bits:
        raise ValueError("pack_rows: a residue does not fit %d bits" % bits)
    pos = np.arange(n, dtype=np.uint64) * np.uint64(bits)
    wd, sh = (pos >> np.uint64(6)).astype(np.intp), pos & np.uint64(63)
    nw = n * bits // 64
    flat = w.reshape(-1, n)
    # bits < 64: a coefficient starts in every word, so the coefficients that start in word w are a run [start[w], start[w + 1]).  Their fields are disjoint
    # (the sums are ORs): word w = their low parts + what the last coefficient that starts in word w - 1 spills over
    start = np.searchsorted(wd, np.arange(nw))
    low = np.add.reduceat(flat << sh, start, axis=1)
    spill = np.add.reduceat((flat >> (np.uint64(63) - sh)) >> np.uint64(1), start, axis=1)       # v >> (64 - sh), 0 for sh = 0
    low[:, 1:] += spill[:, :-1]
    return low.reshape(w.shape[:-1] + (nw,))


def unpack_rows(packed, bits, n):
    """uint64 [..., n * bits / 64] packed rows -> uint64 [..., n] values below 2^bits (NOT reduced: a value may be >= the modulus, the device checks)"""
    p = np.ascontiguousarray(packed, dtype=np.uint64)
    bits, n = int(bits), int(n)
    if not 2 <= bits <= 60 or (n * bits) % 64 or p.shape[-1] != n * bits // 64:
        raise ValueError("unpack_rows: rows of %d words are not %d coefficients of %d bits" % (p.shape[-1], n, bits))
    pos = np.arange(n, dtype=np.uint64) * np.uint64(bits)
    wd, sh = (pos >> np.uint64(6)).astype(np.intp), pos & np.uint64(63)
    flat = np.concatenate([p.reshape(-1, p.shape[-1]), np.zeros((p.size // p.shape[-1], 1), dtype=np.uint64)], axis=1)
    lo = flat[:, wd] >> sh
    hi = (flat[:, wd + 1] << (np.uint64(63) - sh)) << np.uint64(1)                # word << (64 - sh), 0 for sh = 0
    return ((lo | hi) & np.uint64((1 << bits) - 1)).reshape(p.shape[:-1] + (n,))


def packed_bits(q):
    """bit widths of the packed rows of the moduli q"""
    return [int(x).bit_length() for x in q]


def pack_ciphertexts(words, q, n):
    """uint64 [count, polys * k * n] ciphertext words -> packed [count, polys * (n / 64) * sum bits] in [poly][limb] row order"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    k = len(q)
    w = w.reshape(w.shape[0], -1, k, n)
    return np.concatenate([pack_rows(w[:, p, j], b) for p in range(w.shape[1]) for j, b in enumerate(packed_bits(q))], axis=1)


def unpack_ciphertexts(packed, q, n, polys):
    """the inverse of pack_ciphertexts (values are not reduced)"""
    p = np.ascontiguousarray(packed, dtype=np.uint64)
    out, off = [], 0
    for _ in range(polys):
        for b in packed_bits(q):
            out.append(unpack_rows(p[:, off:off + n * b // 64], b, n))
            off += n * b // 64
    if off != p.shape[1]:
        raise ValueError("unpack_ciphertexts: %d words per ciphertext, expected %d" % (p.shape[1], off))
    return np.concatenate(out, axis=1)


# A packed batch: the compact batch with its c0 polynomials as packed rows.
#     8 B magic "CNHIPPK1" | u32 version (1) | 32 B public seed | u64 nonce | u64 first item | u64 count | 32 B parms_id of the level
#     | u32 limbs | limbs x u8 bit widths | IntArray of count * (N / 64) * sum(widths) words: [ciphertext][limb] rows        (all little-endian)
PACKED_MAGIC = b"CNHIPPK1"
PACKED_VERSION = 1


class PackedDescriptor(CompactDescriptor):
    """a CompactDescriptor and the bit widths of the rows (one per limb of the level): what turns packed c0 rows back into ciphertexts"""

    def __init__(self, a_seed, a_nonce, a_item0, count, parms_id, bits):
        super().__init__(a_seed, a_nonce, a_item0, count, parms_id)
        self.bits = [int(b) for b in bits]
        if not self.bits or min(self.bits) < 2 or max(self.bits) > 60:
            raise ValueError("packed rows have 2 .. 60 bits per coefficient")

    def __eq__(self, o):
        return super().__eq__(o) and self.bits == getattr(o, "bits", None)


def save_packed_batch(f, packed, desc):
    """packed c0 rows [count, (n / 64) * sum(desc.bits)] with their PackedDescriptor"""
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    bits = desc.bits
    if packed.ndim != 2 or packed.shape[0] != desc.count or packed.shape[1] % sum(bits):
        raise ValueError("packed words of shape %s do not belong to a descriptor of %d ciphertexts" % (packed.shape, desc.count))
    f.write(PACKED_MAGIC)
    f.write(struct.pack("<I", PACKED_VERSION))
    f.write(desc.a_seed)
    _w_u64(f, desc.a_nonce)
    _w_u64(f, desc.a_item0)
    _w_u64(f, desc.count)
    f.write(desc.parms_id)
    f.write(struct.pack("<I", len(bits)))
    f.write(bytes(bits))
    _w_array(f, packed)


def load_packed_batch(f, parms):
    """(packed c0 rows [count, words], descriptor, limbs); `parms`: the Parameters of the chain's first level - a batch of any of its levels loads.  The
    widths are checked against the level's moduli, the word count against them and the item range; the rows are NOT unpacked (the device reduces and
    reports a residue that is not below its modulus: Context.ct_upload_packed)"""
    if _rd(f, 8) != PACKED_MAGIC:
        raise BadStream("Bad stream format. (not a packed batch)")
    version = struct.unpack("<I", _rd(f, 4))[0]
    if version != PACKED_VERSION:
        raise BadStream("packed batch of version %d (this library reads %d)" % (version, PACKED_VERSION))
    a_seed = _rd(f, 32)
    a_nonce, a_item0, count = _r_u64(f), _r_u64(f), _r_u64(f)
    pid = _rd(f, 32)
    limbs = parms.chain().get(pid)
    if limbs is None:
        raise BadStream("the packed batch belongs to other encryption parameters")
    if (a_item0 + count) >> 40:
        raise BadStream("Bad stream format. (items)")
    nl = struct.unpack("<I", _rd(f, 4))[0]
    if nl != limbs or list(_rd(f, nl)) != packed_bits(parms.q[:limbs]):
        raise BadStream("Bad stream format. (bit widths of the packed rows)")
    row = parms.n // 64 * sum(packed_bits(parms.q[:limbs]))
    words = _r_array(f)
    if words.size != count * row:
        raise BadStream("Bad stream format. (%d words for %d packed ciphertexts of %d limbs)" % (words.size, count, limbs))
    return words.reshape(count, row), PackedDescriptor(a_seed, a_nonce, a_item0, count, pid, packed_bits(parms.q[:limbs])), limbs


class _Prefixed:
    """`head` followed by the rest of the stream `f` (a parms_id read ahead)"""

    def __init__(self, head, f):
        self.head, self.f = head, f

    def read(self, nbytes):
        if self.head:
            out, self.head = self.head[:nbytes], self.head[nbytes:]
            return out + (self.f.read(nbytes - len(out)) if nbytes > len(out) else b"")
        return self.f.read(nbytes)


def save_kswitch_keys(f, parms, dbc, entries):
    """entries: list (dim1) of arrays [digits, 2*k*N] (or None / empty for an absent key)"""
    f.write(parms.parms_id())
    f.write(struct.pack("<i", int(dbc)))
    _w_u64(f, len(entries))
    for e in entries:
        digits = [] if e is None else list(np.asarray(e, dtype=np.uint64).reshape(-1, 2 * parms.k * parms.n))
        _w_u64(f, len(digits))
        for d in digits:
            save_ciphertext(f, d, parms, size=2, is_ntt_form=True)


def load_kswitch_keys(f, parms, expect_dbc=None):
    """-> (decomposition_bit_count, list of arrays [digits, 2*k*N] or None)"""
    if _rd(f, 32) != parms.parms_id():
        raise BadStream("keys are not valid for the encryption parameters")
    dbc = struct.unpack("<i", _rd(f, 4))[0]
    if not 1 <= dbc <= 60 or (expect_dbc is not None and dbc != expect_dbc):
        raise BadStream("keys are not valid for the encryption parameters (decomposition bit count %d)" % dbc)
    dim1 = _r_u64(f)
    if dim1 > parms.n:
        raise BadStream("Bad stream format. (key count)")
    out = []
    for _ in range(dim1):
        dim2 = _r_u64(f)
        if dim2 > 64 * parms.k:
            raise BadStream("Bad stream format. (digit count)")
        out.append(np.stack([load_ciphertext(f, parms, want_ntt_form=True)[0] for _ in range(dim2)]) if dim2 else None)
    return dbc, out


def digit_count(parms, dbc):
    """(limb, digit) pairs of a key-switching key: sum over limbs of ceil(bits(q_l) / dbc)"""
    return sum(-(-q.bit_length() // dbc) for q in parms.q)


# ------------------------------------------------------------------------------------------------ one environment
def _galois_elements(ctx):
    """elements this context holds keys for, ascending (cn_galois_elts): the default set of KeyGenerator.GaloisKeys(dbc), keys generated for a
    network's own steps (cn_keygen_galois) and uploaded ones alike.  A context stand-in that cannot enumerate its keys (the CPU test harness)
    is asked for the default set, 3^(+-2^i) and 2N-1, element by element."""
    if hasattr(ctx, "galois_elts"):
        return ctx.galois_elts()
    m, n = 2 * ctx.n, ctx.n
    cand, g = {m - 1}, 3
    for _ in range(max(1, n.bit_length() - 2)):
        cand.add(g)
        cand.add(pow(g, -1, m))
        g = g * g % m
    return sorted(e for e in cand if ctx.has_galois_key(e))


def save_environment(stream, env, withPrivateKeys=True, noise_standard_deviation=DEFAULT_NOISE_STANDARD_DEVIATION):
    """AtomicSealBfvEncryptedEnvironment.SaveToStream (AtomicSealBfvVector.cs:93-104).  Keys are read back from HBM
    (cn_get_key); the secret key only exists when the client ran on this context (DeviceClient)."""
    ctx = env.ctx
    parms = Parameters(ctx.n, ctx.q, ctx.t, noise_standard_deviation)
    parms.save(stream)
    save_ciphertext(stream, ctx.get_key(2), parms, size=2, is_ntt_form=True)                       # PublicKey
    save_kswitch_keys(stream, parms, ctx.dbc, [ctx.get_key(0).reshape(-1, 2 * parms.k * parms.n)])   # RelinKeys
    elts = _galois_elements(ctx)
    entries = [None] * parms.n if elts else []
    for e in elts:
        entries[(e - 1) // 2] = ctx.get_key(1, e).reshape(-1, 2 * parms.k * parms.n)
    save_kswitch_keys(stream, parms, ctx.gdbc, entries)                                            # GaloisKeys
    if withPrivateKeys:
        save_plaintext(stream, ctx.get_key(3), parms.parms_id())                                   # SecretKey
    else:
        save_plaintext(stream, np.zeros(0, dtype=np.uint64), PARMS_ID_ZERO)                        # new SecretKey()


def load_environment(stream, context_factory, client_factory=None):
    """AtomicSealBfvEncryptedEnvironment.LoadFromStream (AtomicSealBfvVector.cs:106-130): parameters -> context, then the
    keys.  `context_factory(n, t, q, dbc, gdbc)` builds the libcnhip context; the decomposition bit counts come from the key
    streams.  Without a secret key the environment can evaluate but not decrypt (the reference prints a warning)."""
    from .hewrapper import AtomicSealBfvEncryptedEnvironment
    blob = io.BytesIO(stream.read())
    parms = Parameters.load(blob)
    pk, size = load_ciphertext(blob, parms, want_ntt_form=True)
    if size != 2:
        raise BadStream("public key is not valid for the encryption parameters")
    dbc, rl = load_kswitch_keys(blob, parms)
    gdbc, gk = load_kswitch_keys(blob, parms)
    sk = load_plaintext(blob, parms, expect_parms_id=None)
    if len(rl) != 1 or rl[0] is None or rl[0].shape[0] != digit_count(parms, dbc):
        raise BadStream("relinearization keys are not valid for the encryption parameters")
    ctx = context_factory(parms.n, parms.t, parms.q, dbc, gdbc)
    ctx.set_public_key(pk)
    ctx.set_relin_key(rl[0].reshape(-1))
    for i, e in enumerate(gk):
        if e is not None:
            if e.shape[0] != digit_count(parms, gdbc):
                raise BadStream("Galois keys are not valid for the encryption parameters")
            ctx.set_galois_key(2 * i + 1, e.reshape(-1))
    if sk.size:
        if sk.size != parms.k * parms.n:
            raise BadStream("secret key is not valid for the encryption parameters")
        ctx.set_secret_key(sk)
    client = client_factory(ctx) if client_factory is not None else None
    if client is None:
        from .client import DeviceClient
        client = DeviceClient(ctx)
    client.has_secret_key = bool(sk.size)
    return AtomicSealBfvEncryptedEnvironment(ctx, client)


def save_environments(stream, envs, withPrivateKeys):
    """EncryptedSealBfvEnvironment.Save (EncryptedSealBfvVector.cs:104-126): zip, one stored entry per plaintext prime"""
    with zipfile.ZipFile(stream, "w", compression=zipfile.ZIP_STORED) as z:
        for i, e in enumerate(envs):
            mem = io.BytesIO()
            save_environment(mem, e, withPrivateKeys)
            z.writestr("environment%03d" % i, mem.getvalue())
    return stream


def load_environments(stream, context_factory, client_factory=None):
    """EncryptedSealBfvEnvironment(Stream) (EncryptedSealBfvVector.cs:49-68): entries in name order"""
    envs = []
    with zipfile.ZipFile(stream, "r") as z:
        for name in sorted(z.namelist()):
            if not name.startswith("environment"):
                raise BadStream("Bad stream format. (unexpected entry %s)" % name)
            envs.append(load_environment(io.BytesIO(z.read(name)), context_factory, client_factory))
    if not envs:
        raise BadStream("Bad stream format. (no environments)")
    return envs


# ------------------------------------------------------------------------------------------------ vectors / matrices
def _fmt_double(x):
    """Double.ToString() of .NET Framework (15 significant digits, 'E+XX' exponents)"""
    s = "%.15g" % float(x)
    if "e" in s:
        m, e = s.split("e")
        s = "%sE%s%02d" % (m, e[0], int(e[1:]))
    return s


def _readline(s):
    line = s.readline()
    if line == "":
        raise BadStream("Bad stream format.")
    return line.rstrip("\r\n")


def _expect(s, text):
    if _readline(s) != text:
        raise BadStream("Bad stream format.")


def write_atomic_vector(s, vec, env):
    """AtomicSealBfvEncryptedVector.Write (AtomicSealBfvVector.cs:1273-1302); `s` is a text stream.  Ciphertexts are written at their own level
    (the parms_id of q[:l] when the vector was switched down, SEAL's Ciphertext.Save)."""
    ctx = vec.encData.buf.ctx if vec.encData is not None else env.ctx
    parms = Parameters(ctx.n, ctx.q, ctx.t)
    s.write("<Start EncryptedVector>\n")
    s.write(_fmt_double(vec.Scale) + "\n")
    s.write(("True" if vec.IsSigned else "False") + "\n")
    s.write(vec.Format.name + "\n")
    s.write("%d\n" % vec.Dim)
    mem = io.BytesIO()
    if vec.encData is not None:
        cts = ctx.ct_download(vec.encData.h, vec.encData.first, vec.encData.count)
        s.write("Encrypted\n%d\n" % len(cts))
        for c in cts:
            save_ciphertext(mem, c, parms, size=2)
    else:
        if vec.plainDense is not None:
            plains = list(ctx.pt_download(vec.plainDense.h, vec.plainDense.first, vec.plainDense.count))
        else:
            plains = [np.array([x], dtype=np.uint64) for x in vec.plainSparse]     # constant polynomial, CoeffCount 1
        s.write("Plain\n%d\n" % len(plains))
        for p in plains:
            save_plaintext(mem, p)
    s.write(base64.b64encode(mem.getvalue()).decode("ascii") + "\n")
    s.write("<End EncryptedVector>\n")
    s.flush()


def read_atomic_vector(s, env):
    """AtomicSealBfvEncryptedVector.Read (AtomicSealBfvVector.cs:1304-1345).  Ciphertexts may be at any level of `env`'s chain (SEAL 3.2's
    Ciphertext.Load + is_valid_for): the vector then lives at that level - its `Limbs`, environment env.Level(vec.Limbs)."""
    from .hewrapper import AtomicSealBfvEncryptedVector, EVectorFormat, _Buf
    root = getattr(env, "_root", env)
    ctx = root.ctx
    parms = Parameters(ctx.n, ctx.q, ctx.t)
    _expect(s, "<Start EncryptedVector>")
    try:
        scale = float(_readline(s))
        signed = {"True": True, "False": False}[_readline(s)]
        fmt = EVectorFormat[_readline(s)]
        dim = int(_readline(s))
        mode = _readline(s)
        length = int(_readline(s))
        mem = io.BytesIO(base64.b64decode(_readline(s), validate=True))
    except (KeyError, ValueError) as e:
        raise BadStream("Bad stream format. (%s)" % e)
    vec = AtomicSealBfvEncryptedVector._new(Scale=scale, IsSigned=signed, Format=fmt, Dim=dim)
    if length <= 0:
        raise BadStream("Bad stream format. (empty vector)")
    if mode == "Encrypted":
        cts, level = [], None
        for _ in range(length):
            w, size, limbs = load_ciphertext_any_level(mem, parms, want_ntt_form=False)
            if size != 2:
                raise BadStream("Bad stream format. (ciphertext size %d)" % size)
            if level is not None and limbs != level:
                raise BadStream("Bad stream format. (ciphertexts of one vector at different levels)")
            level = limbs
            cts.append(w)
        if level != parms.k:
            ctx = root.Level(level).ctx
        vec.encData = _Buf(ctx, "ct", length).view()
        ctx.ct_upload(vec.encData.h, 0, np.stack(cts))
    elif mode == "Plain":
        plains = [load_plaintext(mem, parms) for _ in range(length)]
        if fmt == EVectorFormat.sparse:
            if any(p.size > 1 for p in plains):
                raise BadStream("Bad stream format. (sparse plaintext with more than one coefficient)")
            vec.plainSparse = [int(p[0]) if p.size else 0 for p in plains]
        else:
            full = np.zeros((length, ctx.n), dtype=np.uint64)
            for i, p in enumerate(plains):
                full[i, :p.size] = p
            vec.plainDense = _Buf(ctx, "pt", length).view()
            ctx.pt_upload(vec.plainDense.h, 0, full)
            vec.plainZero = [not p.any() for p in plains]
    else:
        raise BadStream("unknown format")
    if mem.read(1):
        raise BadStream("Bad stream format. (trailing bytes)")
    _expect(s, "<End EncryptedVector>")
    return vec


def write_vector(s, vec, env):
    """EncryptedSealBfvVector.Write (EncryptedSealBfvVector.cs:430-439)"""
    s.write("<Start LargeEncryptedVector>\n")
    s.write(_fmt_double(vec.Scale) + "\n")
    s.write("%d\n" % len(vec.eVectors))
    for a, e in zip(vec.eVectors, env.Environments):
        write_atomic_vector(s, a, e)
    s.write("<End LargeEncryptedVector>\n")
    s.flush()


def read_vector(s, env):
    """EncryptedSealBfvVector.Read (EncryptedSealBfvVector.cs:414-429)"""
    from .hewrapper import EncryptedSealBfvVector
    _expect(s, "<Start LargeEncryptedVector>")
    try:
        scale = float(_readline(s))
        count = int(_readline(s))
    except ValueError as e:
        raise BadStream("Bad stream format. (%s)" % e)
    if count != len(env.Environments):
        raise BadStream("Bad stream format. (%d plaintext primes, environment has %d)" % (count, len(env.Environments)))
    atoms = [read_atomic_vector(s, e) for e in env.Environments]
    _expect(s, "<End LargeEncryptedVector>")
    return EncryptedSealBfvVector._of(atoms, scale)


def write_matrix(s, mat, env):
    """EncryptedSealBfvMatrix.Write (EncryptedSealBfvMatrix.cs:199-208)"""
    s.write("<Start LargeEncryptedMatrix>\n")
    s.write(mat.Format.name + "\n")
    s.write("%d\n" % len(mat.leVectors))
    for v in mat.leVectors:
        write_vector(s, v, env)
    s.write("<End LargeEncryptedMatrix>\n")
    s.flush()


def read_matrix(s, env):
    """EncryptedSealBfvMatrix.Read (EncryptedSealBfvMatrix.cs:182-197)"""
    from .hewrapper import EMatrixFormat, EncryptedSealBfvMatrix
    _expect(s, "<Start LargeEncryptedMatrix>")
    try:
        fmt = EMatrixFormat[_readline(s)]
        count = int(_readline(s))
    except (KeyError, ValueError) as e:
        raise BadStream("Bad stream format. (%s)" % e)
    vecs = [read_vector(s, env) for _ in range(count)]
    _expect(s, "<End LargeEncryptedMatrix>")
    return EncryptedSealBfvMatrix(vecs, env, CopyVectors=False, Format=fmt)
