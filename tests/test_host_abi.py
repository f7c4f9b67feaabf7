"""The C ABI as a whole, host only: vqvae_amd._lib.HEADERS against the headers under include/, the built library, the C
compiler's view of every mirrored struct and macro, and the Makefile's object rule.  One check per property, run for
every header; what is specific to one feature (its literal NAMES, the words its header must contain, its C-side
validation) stays in that feature's own test file."""
import ctypes as C
import itertools
import os

import pytest

import abi_headers as A
from vqvae_amd import _lib

FILES = list(_lib.HEADERS)
BASE = 'vqvae_hip.h'

# adding an export is a deliberate edit of this table
EXPORT_COUNTS = {'vqvae_hip.h': 128, 'vqvae_codebook.h': 3, 'vqvae_vq_ema.h': 5, 'vqvae_kmeans.h': 6, 'vqvae_optim.h': 6,
                 'vqvae_sampling.h': 3, 'vqvae_gen_slots.h': 3, 'vqvae_gen_cond.h': 2, 'vqvae_gen_rng.h': 5,
                 'vqvae_corpus.h': 2, 'vqvae_ingest.h': 5, 'vqvae_ragged.h': 5, 'vqvae_metrics.h': 5, 'vqvae_pitch.h': 5,
                 'vqvae_ragged_decoder.h': 9, 'vqvae_align.h': 7, 'vqvae_codes.h': 9}

# what load() calls each header when its version is not the bound one
VERSION_WORDS = {'vqvae_hip.h': 'ABI', 'vqvae_codebook.h': 'codebook ABI', 'vqvae_vq_ema.h': 'EMA-codebook ABI',
                 'vqvae_kmeans.h': 'k-means ABI', 'vqvae_optim.h': 'optimizer-hook ABI', 'vqvae_sampling.h': 'sampling ABI',
                 'vqvae_gen_slots.h': 'slot-generation ABI', 'vqvae_gen_cond.h': 'latent-condition ABI',
                 'vqvae_gen_rng.h': 'device-uniforms ABI', 'vqvae_corpus.h': 'resident-corpus ABI',
                 'vqvae_ingest.h': 'ingest ABI', 'vqvae_ragged.h': 'ragged-front-end ABI',
                 'vqvae_metrics.h': 'audio-metrics ABI', 'vqvae_pitch.h': 'pitch ABI',
                 'vqvae_ragged_decoder.h': 'ragged-decoder ABI', 'vqvae_align.h': 'alignment ABI',
                 'vqvae_codes.h': 'code-statistics ABI'}

# typedef'd structs of the headers that _lib mirrors with no Structure, and where they are read instead
READ_ELSEWHERE = {'vqvae_ingest_bounds': 'vqvae_amd/ingest.py reads the array back as four int32 words per utterance'}


def _integers():
    return {n: v for n, v in vars(_lib).items() if n.isupper() and type(v) is int}


def _header_of(constant):
    """The rule of _lib's docstring: the header whose stem is the longest prefix of the name, else vqvae_hip.h."""
    stems = {f[len('vqvae_'):-len('.h')].upper() + '_': f for f in FILES if f != BASE}
    match = [s for s in stems if constant.startswith(s)]
    return stems[max(match, key=len)] if match else BASE


def _structures():
    return [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]


@pytest.fixture(scope='module')
def compiled(tmp_path_factory):
    """What the host C compiler makes of every mirrored struct and every mirrored macro, from one program."""
    lines = []
    for cls in _structures():
        t = cls._c_name_
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (t, t))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (t, f, t, f, t, f))
    for n in _integers():
        if 'VQVAE_' + n in A.macros(_header_of(n)):
            lines.append('printf("VQVAE_%s %%lld\\n", (long long)(VQVAE_%s));' % (n, n))
    return A.run_c99(lines, tmp_path_factory.mktemp('abi'))


def test_the_registry_is_the_include_directory():
    assert FILES[0] == BASE and sorted(FILES) == sorted(os.listdir(A.INCLUDE))
    assert all(h.file == f for f, h in _lib.HEADERS.items())
    assert _lib.PROTOTYPES is _lib.HEADERS[BASE].prototypes and _lib.ABI_VERSION == _lib.HEADERS[BASE].version == 5


def test_export_counts_are_pinned():
    assert {f: len(A.exports(f)) for f in FILES} == EXPORT_COUNTS
    assert sum(EXPORT_COUNTS.values()) == 208


def test_no_symbol_is_in_two_tables():
    for a, b in itertools.combinations(_lib.HEADERS.values(), 2):
        assert not set(a.prototypes) & set(b.prototypes), (a.file, b.file)


@pytest.mark.parametrize('file', FILES)
def test_exports_and_prototypes(file):
    table = _lib.HEADERS[file].prototypes
    assert set(A.exports(file)) == set(table), set(A.exports(file)) ^ set(table)
    lib = _lib.load()
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert A.param_count(file, name) == len(args), (name, A.prototype(file, name))


@pytest.mark.parametrize('file', FILES)
def test_version_is_bound_and_a_mismatch_is_an_import_error(file, monkeypatch):
    h = _lib.HEADERS[file]
    assert h.version_symbol == ('vqvae_abi_version' if file == BASE else 'vqvae_%s_abi_version' % file[len('vqvae_'):-2])
    assert h.version_symbol in h.prototypes and h.words == VERSION_WORDS[file]
    assert getattr(_lib.load(), h.version_symbol)() == h.version == (5 if file == BASE else 1)     # a bump is a deliberate edit
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setitem(_lib.HEADERS, file, h._replace(version=h.version + 1))
    with pytest.raises(ImportError) as e:
        _lib.load()
    binds = 'ABI %d' if file == BASE else '%d'
    assert str(e.value) == ('libvqvae_hip.so at %s has %s %d, this package binds ' + binds + ': rebuild it (__graft_entry__.build())') \
        % (_lib.LIB_PATH, VERSION_WORDS[file], h.version, h.version + 1)
    assert _lib._lib is None


def test_a_missing_symbol_is_an_attribute_error_before_any_version_is_compared(monkeypatch):
    first, last = _lib.HEADERS[BASE], _lib.HEADERS[FILES[-1]]
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setitem(_lib.HEADERS, BASE, first._replace(version=first.version + 1))
    monkeypatch.setitem(_lib.HEADERS, last.file, last._replace(prototypes=dict(last.prototypes, vqvae_no_such_symbol=(C.c_int, []))))
    with pytest.raises(AttributeError, match='vqvae_no_such_symbol'):
        _lib.load()


@pytest.mark.parametrize('file', FILES)
def test_constants_equal_the_macros_as_compiled(file, compiled):
    mine = {n: v for n, v in _integers().items() if n not in dict(_lib.UNMIRRORED) and _header_of(n) == file}
    for n, v in mine.items():
        assert 'VQVAE_' + n in A.macros(file), '%s: _lib.%s mirrors no macro of this header' % (file, n)
        assert compiled['VQVAE_' + n] == [v], n


def test_every_integer_constant_has_exactly_one_home():
    exempt = dict(_lib.UNMIRRORED)
    assert len(exempt) == len(_lib.UNMIRRORED) and all(why for why in exempt.values())
    assert set(exempt) <= set(_integers())
    for n in _integers():
        homes = [f for f in FILES if 'VQVAE_' + n in A.macros(f)]
        assert homes == ([] if n in exempt else [_header_of(n)]), (n, homes)


def test_struct_layouts_are_the_compiler_s(compiled):
    declared = {name: fields for f in FILES for name, fields in A.structs(f).items()}
    mirrored = {cls._c_name_: cls for cls in _structures()}
    assert len(mirrored) == len(_structures()) == 25
    assert set(declared) == set(mirrored) | set(READ_ELSEWHERE) and not set(mirrored) & set(READ_ELSEWHERE)
    for t, cls in mirrored.items():
        assert [f for f, _ in cls._fields_] == declared[t], t
        assert compiled[t] == [C.sizeof(cls)], t
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert compiled['%s.%s' % (t, f)] == [d.offset, d.size], (t, f)


def test_every_object_depends_on_every_header():
    have = {os.path.normpath(os.path.join(A.CSRC, p)) for p in A.object_rule_prerequisites()}
    want = {os.path.join(d, h) for d in (A.CSRC, A.INCLUDE) for h in os.listdir(d) if h.endswith('.h')}
    assert want and want <= have, sorted(want - have)
