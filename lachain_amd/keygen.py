"""lachain_amd/keygen.py — Python mirror of Lachain.Consensus.ThresholdKeygen (the trustless DKG) on liblachain_bls.so.
Class and method names follow the reference:

  TrustlessKeygen            src/Lachain.Consensus/ThresholdKeygen/TrustlessKeygen.cs:19-296
  State                      ThresholdKeygen/Data/State.cs:10-80
  Commitment                 ThresholdKeygen/Data/Commitment.cs:9-79
  BiVarSymmetricPolynomial   ThresholdKeygen/Data/BiVarSymmetricPolynomial.cs:9-60
  CommitMessage / ValueMessage / ThresholdKeyring   ThresholdKeygen/Data/*.cs

Fr arithmetic is Python integers mod r (host code, like the other mirrors).  Every group or envelope operation goes
through the batched library calls: Commit through lcb_g1_mul_batch(generator), the row check through
lcb_dkg_commitment_rows + lcb_g1_mul_batch, the value check through lcb_dkg_commitment_eval + lcb_g1_mul_batch,
TryGetKeys through lcb_dkg_commitment_rows(x = 0) + lcb_g1_eval_poly_batch, the envelopes through
lcb_secp256k1_encrypt_batch / lcb_secp256k1_decrypt_batch.

Besides the reference's per-message handlers there are HandleCommits(list) and HandleSendValues(list): many messages
in one set of batched calls, with the per-message outcomes of the handlers called in the list's order.  An outcome is
the handler's return value, or the exception it would have raised (ArgumentException for the reference's
ArgumentException, CryptoException where Secp256K1Decrypt or Fr.FromBytes throws) as a value.

Commitment.Index and BiVarSymmetricPolynomial.Index are mirrored exactly as written: i (i + 1) / 2 + j for i <= j makes
some index pairs share a coefficient (k_dkg.hip's dkg_index follows it too).
"""
import secrets
import struct

from . import native, threshold_signature, tpke
from .mcl import Fr, G1

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


class ArgumentException(ValueError):
    """the reference's ArgumentException (its message is the reference's)"""


class CryptoException(ValueError):
    """Secp256K1Decrypt, Fr.FromBytes or an array index threw in the reference"""


def fr_to_bytes(v: int) -> bytes:
    return (v % R).to_bytes(32, "little")


def fr_from_bytes(b: bytes) -> int:
    v = int.from_bytes(b, "little")
    if len(b) != 32 or v >= R:
        raise CryptoException("Fr.FromBytes: invalid encoding")
    return v


def _index(i: int, j: int) -> int:
    if i > j:
        i, j = j, i
    return i * (i + 1) // 2 + j


def _eval_poly(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


class _SystemRng:
    """the default source of polynomial coefficients, ephemeral keys and nonces: the operating system's CSPRNG"""

    @staticmethod
    def randbelow(n):
        return secrets.randbelow(n)

    @staticmethod
    def randbytes(n):
        return secrets.token_bytes(n)


class _SeededRng:
    """adapter for a random.Random (reproducible tests only: never for real keys)"""

    def __init__(self, rng):
        self._rng = rng

    def randbelow(self, n):
        return self._rng.randrange(n)

    def randbytes(self, n):
        return self._rng.randbytes(n)


def _rng_of(rng):
    return _SystemRng if rng is None else (rng if hasattr(rng, "randbelow") else _SeededRng(rng))


class EcdsaKeyPair:
    def __init__(self, private_key: bytes, public_key: bytes = None):
        self.PrivateKey = bytes(private_key)
        if public_key is None:
            pub, ok = native.ecdsa_pubkey_batch(self.PrivateKey)
            if ok != b"\x01":
                raise ValueError("invalid secp256k1 private key")
            public_key = pub
        self.PublicKey = bytes(public_key)


class Commitment:
    def __init__(self, g1):
        self._coefficients = [bytes(c) for c in g1]
        self.Degree = 0
        while (self.Degree + 1) * (self.Degree + 2) // 2 < len(self._coefficients):
            self.Degree += 1
        if (self.Degree + 1) * (self.Degree + 2) // 2 != len(self._coefficients):
            raise ArgumentException("Invalid length of coefficient vector")

    def Evaluate(self, x: int, y: int = None):
        """Evaluate(x, y): one serialized G1; Evaluate(x): the row of Degree + 1 serialized G1"""
        if y is None:
            row = native.dkg_commitment_rows([self._coefficients], self.Degree, [(0, x)])[0]
        else:
            row = native.dkg_commitment_eval([self._coefficients], self.Degree, [(0, x, y)])[0]
        if row is None:
            raise CryptoException("malformed commitment coefficient")
        return row

    Index = staticmethod(_index)

    def ToBytes(self) -> bytes:
        return b"".join(self._coefficients)

    @staticmethod
    def FromBytes(buffer: bytes):
        buffer = bytes(buffer)
        if len(buffer) % 48:
            raise CryptoException("G1.FromBytes: invalid encoding")
        coeffs = [buffer[o:o + 48] for o in range(0, len(buffer), 48)]
        for c in coeffs:
            G1.FromBytes(c)          # throws on malformed input, as the reference's deserialisation
        return Commitment(coeffs)

    def IsValid(self) -> bool:
        if len(self._coefficients) != (self.Degree + 1) * (self.Degree + 2) // 2:
            return False
        try:
            return all(G1.FromBytes(c).IsValid() for c in self._coefficients)
        except (ValueError, RuntimeError):
            return False

    def __eq__(self, o):
        return isinstance(o, Commitment) and o._coefficients == self._coefficients

    def __hash__(self):
        return hash(tuple(self._coefficients))


class BiVarSymmetricPolynomial:
    def __init__(self, degree: int, c):
        self._coefficients = [int(v) % R for v in c]
        self._degree = degree
        if len(self._coefficients) != (degree + 2) * (degree + 1) // 2:
            raise ArgumentException("Wrong number of coefficients")

    @staticmethod
    def Random(degree: int, rng=None):
        rng = _rng_of(rng)
        return BiVarSymmetricPolynomial(degree, [rng.randbelow(R) for _ in range((degree + 2) * (degree + 1) // 2)])

    def Commit(self) -> Commitment:
        return Commitment(native.mul_batch(1, None, [fr_to_bytes(c) for c in self._coefficients], generator=True))

    def Evaluate(self, x: int):
        row = []
        for i in range(self._degree + 1):
            acc, x_pow_j = 0, 1
            for j in range(self._degree + 1):
                acc = (acc + self._coefficients[_index(i, j)] * x_pow_j) % R
                x_pow_j = x_pow_j * x % R
            row.append(acc)
        return row

    Index = staticmethod(_index)


class CommitMessage:
    def __init__(self, Commitment, EncryptedRows):
        self.Commitment = Commitment
        self.EncryptedRows = list(EncryptedRows)


class ValueMessage:
    def __init__(self, Proposer: int, EncryptedValues):
        self.Proposer = Proposer
        self.EncryptedValues = list(EncryptedValues)


class State:
    def __init__(self, n: int):
        self.Commitment = None
        self.Values = [0] * n
        self.Acks = [False] * n

    def ValueCount(self) -> int:
        return sum(1 for a in self.Acks if a)

    def InterpolateValues(self) -> int:
        if self.Commitment is None:
            raise ArgumentException("Cannot interpolate without commitment")
        need = self.Commitment.Degree + 1
        pts = [(i + 1, self.Values[i]) for i, a in enumerate(self.Acks) if a][:need]
        if len(pts) != need:
            raise RuntimeError("Cannot interpolate values")
        total = 0                                  # MclBls12381.LagrangeInterpolate: the value at 0
        for k, (xk, yk) in enumerate(pts):
            num = den = 1
            for m, (xm, _) in enumerate(pts):
                if m != k:
                    num = num * xm % R
                    den = den * (xm - xk) % R
            total = (total + yk * num * pow(den, -1, R)) % R
        return total

    def ToBytes(self) -> bytes:
        commitment = self.Commitment.ToBytes() if self.Commitment is not None else b""
        return struct.pack("<i", len(commitment)) + commitment + struct.pack("<i", len(self.Acks)) + \
            b"".join(fr_to_bytes(v) for v in self.Values) + bytes(1 if a else 0 for a in self.Acks)

    @staticmethod
    def FromBytes(b: bytes):
        b = bytes(b)
        (c_len,) = struct.unpack_from("<i", b, 0)
        commitment = Commitment.FromBytes(b[4:4 + c_len]) if c_len else None
        (n,) = struct.unpack_from("<i", b, 4 + c_len)
        s = State(n)
        s.Commitment = commitment
        for i in range(n):
            s.Values[i] = fr_from_bytes(b[8 + c_len + 32 * i:8 + c_len + 32 * i + 32])
            s.Acks[i] = b[8 + c_len + 32 * n + i] != 0
        return s

    def __eq__(self, o):
        return isinstance(o, State) and (o.Values, o.Acks, o.Commitment) == (self.Values, self.Acks, self.Commitment)


class ThresholdKeyring:
    def __init__(self, tpke_private_key, tpke_public_key, tpke_verification_public_keys, ts_public_key_set,
                 ts_private_key):
        self.TpkePrivateKey = tpke_private_key
        self.TpkePublicKey = tpke_public_key
        self.TpkeVerificationPublicKeys = tpke_verification_public_keys
        self.ThresholdSignaturePublicKeySet = ts_public_key_set
        self.ThresholdSignaturePrivateKey = ts_private_key

    def PublicPartHash(self) -> bytes:
        return _keyring_hash(self.TpkePublicKey, self.ThresholdSignaturePublicKeySet)


def _keyring_hash(tpke_key, ts_keys) -> bytes:
    ts_bytes = struct.pack("<i", ts_keys.Threshold) + b"".join(k.RawKey for k in ts_keys.Keys)
    return native.keccak256_batch([tpke_key.ToBytes() + ts_bytes])


class TrustlessKeygen:
    def __init__(self, keyPair: EcdsaKeyPair, publicKeys, f: int, cycle: int, rng=None):
        self._keyPair = keyPair
        self._publicKeys = [bytes(p) for p in publicKeys]
        self.Players = len(self._publicKeys)
        self.Faulty = f
        self.Cycle = cycle
        self._myIdx = self._publicKeys.index(keyPair.PublicKey)
        self._keyGenStates = [State(self.Players) for _ in range(self.Players)]
        self._finished = []
        self._confirmations = {}
        self._confirmSent = False
        self._rng = _rng_of(rng)

    # ------------------------------------------------------------ envelopes
    def _encrypt(self, recipients, plaintexts):
        """one batched Secp256K1Encrypt; the ephemeral keys and nonces are drawn here, each used once"""
        n = len(plaintexts)
        eph = b"".join((1 + self._rng.randbelow(SECP_N - 1)).to_bytes(32, "big") for _ in range(n))
        envs, ok = native.secp256k1_encrypt_batch(b"".join(recipients), eph, self._rng.randbytes(16 * n), plaintexts)
        return envs

    def _decrypt(self, envelopes):
        plain, _ = native.secp256k1_decrypt_batch(self._keyPair.PrivateKey, envelopes, [0] * len(envelopes))
        return plain

    # ------------------------------------------------------------ the protocol
    def StartKeygen(self) -> CommitMessage:
        poly = BiVarSymmetricPolynomial.Random(self.Faulty, self._rng)
        commitment = poly.Commit()
        rows = [b"".join(fr_to_bytes(v) for v in poly.Evaluate(i)) for i in range(1, self.Players + 1)]
        envs = self._encrypt(self._publicKeys, rows)
        if any(e is None for e in envs):
            raise CryptoException("Secp256K1Encrypt: invalid public key")
        return CommitMessage(commitment, envs)

    def GetSenderByPublicKey(self, publicKey: bytes) -> int:
        try:
            return self._publicKeys.index(bytes(publicKey))
        except ValueError:
            return -1

    def HandleCommit(self, sender: int, message: CommitMessage) -> ValueMessage:
        out = self.HandleCommits([(sender, message)])[0]
        if isinstance(out, Exception):
            raise out
        return out

    def HandleCommits(self, items):
        """items: (sender, CommitMessage) in handling order -> ValueMessage or exception value per item"""
        out = [None] * len(items)
        live = []
        for k, (sender, message) in enumerate(items):
            if len(message.EncryptedRows) != self.Players:
                out[k] = ArgumentException("")
            elif self._keyGenStates[sender].Commitment is not None:
                out[k] = ArgumentException(f"Double commit from sender {sender}")
            else:
                self._keyGenStates[sender].Commitment = message.Commitment
                live.append(k)
        # Commitment.Evaluate(myIdx + 1) of every live message, one call per degree
        committed = {}
        for degree in sorted({items[k][1].Commitment.Degree for k in live}):
            ks = [k for k in live if items[k][1].Commitment.Degree == degree]
            rows = native.dkg_commitment_rows([items[k][1].Commitment._coefficients for k in ks], degree,
                                              [(q, self._myIdx + 1) for q in range(len(ks))])
            committed.update(zip(ks, rows))
        plain = self._decrypt([items[k][1].EncryptedRows[self._myIdx] for k in live]) if live else []
        my_rows = {}
        for k, p in zip(live, plain):
            if committed[k] is None:
                out[k] = CryptoException("malformed commitment coefficient")
            elif p is None:
                out[k] = CryptoException("Secp256K1Decrypt failed")
            else:
                try:
                    my_rows[k] = [fr_from_bytes(p[o:o + 32]) for o in range(0, len(p), 32)]
                except CryptoException as e:
                    out[k] = e
        ks = list(my_rows)
        scalars = [fr_to_bytes(v) for k in ks for v in my_rows[k]]
        flat = native.mul_batch(1, None, scalars, generator=True) if scalars else []
        pos, good = 0, []
        for k in ks:
            mine = flat[pos:pos + len(my_rows[k])]
            pos += len(my_rows[k])
            if mine != committed[k]:
                out[k] = ArgumentException("Commitment does not match")
            else:
                good.append(k)
        values = [fr_to_bytes(_eval_poly(my_rows[k], i + 1)) for k in good for i in range(self.Players)]
        envs = self._encrypt(self._publicKeys * len(good), values) if good else []
        for q, k in enumerate(good):
            mine = envs[q * self.Players:(q + 1) * self.Players]
            out[k] = ValueMessage(items[k][0], mine) if all(e is not None for e in mine) else \
                CryptoException("Secp256K1Encrypt: invalid public key")
        return out

    def HandleSendValue(self, sender: int, message: ValueMessage) -> bool:
        out = self.HandleSendValues([(sender, message)])[0]
        if isinstance(out, Exception):
            raise out
        return out

    def HandleSendValues(self, items):
        """items: (sender, ValueMessage) in handling order -> the handler's bool or exception value per item"""
        out = [None] * len(items)
        live, acked = [], set()
        for k, (sender, message) in enumerate(items):
            if self._keyGenStates[message.Proposer].Acks[sender] or (message.Proposer, sender) in acked:
                out[k] = ArgumentException("Already handled this value")
                continue
            acked.add((message.Proposer, sender))
            if self._myIdx >= len(message.EncryptedValues):
                out[k] = CryptoException("EncryptedValues: index out of range")
            else:
                live.append(k)
        plain = self._decrypt([items[k][1].EncryptedValues[self._myIdx] for k in live]) if live else []
        values = {}
        for k, p in zip(live, plain):
            if p is None:
                out[k] = CryptoException("Secp256K1Decrypt failed")
                continue
            try:
                values[k] = fr_from_bytes(p)
            except CryptoException as e:
                out[k] = e
                continue
            if self._keyGenStates[items[k][1].Proposer].Commitment is None:
                out[k] = ArgumentException("Cannot handle value since there was no commitment yet")
                del values[k]
        # Commitment.Evaluate(myIdx + 1, sender + 1) against G * value, one call per degree
        ks = list(values)
        expect = {}
        comm_of = lambda k: self._keyGenStates[items[k][1].Proposer].Commitment
        for degree in sorted({comm_of(k).Degree for k in ks}):
            kd = [k for k in ks if comm_of(k).Degree == degree]
            proposers = sorted({items[k][1].Proposer for k in kd})
            slot = {p: q for q, p in enumerate(proposers)}
            got = native.dkg_commitment_eval([self._keyGenStates[p].Commitment._coefficients for p in proposers], degree,
                                             [(slot[items[k][1].Proposer], self._myIdx + 1, items[k][0] + 1) for k in kd])
            expect.update(zip(kd, got))
        mine = dict(zip(ks, native.mul_batch(1, None, [fr_to_bytes(values[k]) for k in ks], generator=True))) if ks else {}
        accepted = set()
        for k in ks:
            if expect[k] is None:
                out[k] = CryptoException("malformed commitment coefficient")
            elif expect[k] != mine[k]:
                out[k] = ArgumentException("Decrypted value does not match commitment")
            else:
                accepted.add(k)
        # the state updates and return values, in handling order (the ack is set even where the handler throws)
        for k, (sender, message) in enumerate(items):
            state = self._keyGenStates[message.Proposer]
            if isinstance(out[k], ArgumentException) and out[k].args == ("Already handled this value",):
                continue
            state.Acks[sender] = True
            if k not in accepted:
                continue
            state.Values[sender] = values[k]
            if state.ValueCount() > 2 * self.Faulty and message.Proposer not in self._finished:
                self._finished.append(message.Proposer)
            if self._confirmSent or not self.Finished():
                out[k] = False
            else:
                self._confirmSent = True
                out[k] = True
        return out

    def HandleConfirm(self, tpkeKey, tsKeys) -> bool:
        h = _keyring_hash(tpkeKey, tsKeys)
        self._confirmations[h] = self._confirmations.get(h, 0) + 1
        return self._confirmations[h] == self.Players - self.Faulty

    def Finished(self) -> bool:
        return sum(1 for s in self._keyGenStates if s.ValueCount() > 2 * self.Faulty) > self.Faulty

    def TryGetKeys(self):
        if not self.Finished():
            return None
        dealers = self._finished[:self.Faulty + 1]
        states = [self._keyGenStates[d] for d in dealers]
        if any(s.ValueCount() <= 2 * self.Faulty for s in states):
            raise RuntimeError("Impossible")
        pub_key_poly = [G1.Zero() for _ in range(self.Faulty + 1)]
        secret_key = 0
        rows = {}
        for degree in sorted({s.Commitment.Degree for s in states}):
            sd = [q for q, s in enumerate(states) if s.Commitment.Degree == degree]
            got = native.dkg_commitment_rows([states[q].Commitment._coefficients for q in sd], degree,
                                             [(i, 0) for i in range(len(sd))])
            rows.update(zip(sd, got))
        for q, s in enumerate(states):
            if rows[q] is None:
                raise CryptoException("malformed commitment coefficient")
            for i, x in enumerate(rows[q]):
                pub_key_poly[i] = pub_key_poly[i] + G1.FromBytes(x)
            secret_key = (secret_key + s.InterpolateValues()) % R
        pub_keys = native.g1_eval_poly_batch([p.ToBytes() for p in pub_key_poly], list(range(self.Players + 1)))
        sk = Fr.FromBytes(fr_to_bytes(secret_key))
        return ThresholdKeyring(
            tpke.PrivateKey(sk, self._myIdx),
            tpke.PublicKey(pub_keys[0], self.Faulty),
            [tpke.PublicKey(x, self.Faulty) for x in pub_keys[1:]],
            threshold_signature.PublicKeySet([threshold_signature.PublicKey(x) for x in pub_keys[1:]], self.Faulty),
            threshold_signature.PrivateKeyShare(sk))

    # ------------------------------------------------------------ persistence (TrustlessKeygen.cs:195-260)
    def ToBytes(self) -> bytes:
        out = struct.pack("<iiQ", self.Players, self.Faulty, self.Cycle) + b"".join(self._publicKeys)
        for s in self._keyGenStates:
            b = s.ToBytes()
            out += struct.pack("<i", len(b)) + b
        out += struct.pack("<i", len(self._finished)) + b"".join(struct.pack("<i", f) for f in self._finished)
        out += struct.pack("<i", len(self._confirmations))
        for h, count in self._confirmations.items():
            out += h + struct.pack("<i", count)
        return out + bytes([1 if self._confirmSent else 0])

    @staticmethod
    def FromBytes(b: bytes, keyPair: EcdsaKeyPair, rng=None):
        b = bytes(b)
        players, faulty, cycle = struct.unpack_from("<iiQ", b, 0)
        keys = [b[16 + 33 * i:16 + 33 * i + 33] for i in range(players)]
        kg = TrustlessKeygen(keyPair, keys, faulty, cycle, rng)
        offset = 16 + 33 * players
        for i in range(players):
            (ln,) = struct.unpack_from("<i", b, offset)
            kg._keyGenStates[i] = State.FromBytes(b[offset + 4:offset + 4 + ln])
            offset += 4 + ln
        (cnt,) = struct.unpack_from("<i", b, offset)
        kg._finished = list(struct.unpack_from("<%di" % cnt, b, offset + 4))
        offset += 4 + 4 * cnt
        (cnt,) = struct.unpack_from("<i", b, offset)
        offset += 4
        for _ in range(cnt):
            kg._confirmations[b[offset:offset + 32]] = struct.unpack_from("<i", b, offset + 32)[0]
            offset += 36
        kg._confirmSent = b[offset] != 0
        return kg

    def __eq__(self, o):
        return isinstance(o, TrustlessKeygen) and \
            (self._keyPair.PrivateKey, self._publicKeys, self._myIdx, self._keyGenStates, self._finished,
             self._confirmations, self._confirmSent, self.Faulty, self.Players, self.Cycle) == \
            (o._keyPair.PrivateKey, o._publicKeys, o._myIdx, o._keyGenStates, o._finished, o._confirmations,
             o._confirmSent, o.Faulty, o.Players, o.Cycle)
