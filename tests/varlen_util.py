"""Variable-length FASTQ for the --variable-length tests: a text of reads of different lengths and its twin, the same records
padded to L -- 'N' behind each read's end, the quality offset character under it.  Names are unique per record, so a record's
true length can be looked up by its name."""
import numpy as np

from scalce_amd import synth


def lengths_covering(n, L, seed, lo=0):
    """n lengths in lo .. L: every value at least once (n permitting), the rest uniform, shuffled -- records of every size
    follow one another, so record starts fall on every byte phase of 16."""
    rng = np.random.default_rng(seed)
    every = np.arange(lo, L + 1)
    if len(every) > n:
        every = rng.choice(every, size=n, replace=False)
    lens = np.concatenate([every, rng.integers(lo, L + 1, size=n - len(every))])
    rng.shuffle(lens)
    return lens.astype(np.int64)


def texts(L, lens, seed, names=None, prefix="v.", suffix="", n_frac=0.01, phred=33):
    """(variable text, padded twin, names) for len(lens) records: bases and qualities from synth.reads_and_quals."""
    n = len(lens)
    bases, quals = synth.reads_and_quals(n, max(L, 1), seed=seed, n_frac=n_frac, dup_frac=0.1)
    bases, quals = bases[:, :L], quals[:, :L] + (phred - 33)
    if names is None:
        names = [(prefix + str(i) + suffix).encode() for i in range(n)]
    assert len(set(names)) == n
    var, pad = [], []
    for i in range(n):
        k = int(lens[i])
        b, q = bases[i].tobytes(), quals[i].tobytes()
        var.append(b"@" + names[i] + b"\n" + b[:k] + b"\n+\n" + q[:k] + b"\n")
        pad.append(b"@" + names[i] + b"\n" + b[:k] + b"N" * (L - k) + b"\n+\n" + q[:k] + bytes([phred]) * (L - k) + b"\n")
    return b"".join(var), b"".join(pad), names


def records_of(text):
    """the four-line records of a FASTQ text"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def cut_to_lengths(padded_text, length_of_name):
    """every record of a padded text cut to its true length, looked up by name (the name line without '@' up to a blank)"""
    out = []
    for rec in records_of(padded_text):
        name, seq, plus, qual = rec[:-1].split(b"\n")
        k = length_of_name[name[1:].split(b" ")[0]]
        out.append(name + b"\n" + seq[:k] + b"\n" + plus + b"\n" + qual[:k] + b"\n")
    return b"".join(out)
