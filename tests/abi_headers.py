"""What the C headers under include/ say, read once for every ABI test: the functions a header declares and how many
parameters each takes, its macros and typedef'd structs, the make database of csrc/, and a host C compiler that
evaluates what a regex cannot (a macro's value, a struct's layout)."""
import functools
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')


@functools.lru_cache(maxsize=None)
def code(header):
    """The header's text without its comments."""
    text = open(os.path.join(INCLUDE, header)).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def exports(header):
    """Sorted names of the functions the header declares."""
    return sorted(set(re.findall(r'\b(vqvae_[a-z0-9_]+)\s*\(', code(header))))


def prototype(header, name):
    """The parameter list of one declaration, as written."""
    found = re.findall(r'\b%s\s*\(([^()]*)\)\s*;' % name, code(header))
    assert len(found) == 1, (header, name, found)
    return found[0]


def param_count(header, name):
    params = prototype(header, name).strip()
    return 0 if params == 'void' else len(params.split(','))


def macros(header):
    """Names of the object-like macros the header defines, the include guard aside."""
    return [m for m in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VQVAE_\w+)', code(header), flags=re.M) if not m.endswith('_H_')]


def structs(header):
    """{name: [field names in order]} of the structs the header typedefs."""
    found = {}
    for body, name in re.findall(r'typedef\s+struct[^{;]*\{([^}]*)\}\s*(\w+)\s*;', code(header)):
        found[name] = [re.findall(r'\w+', re.sub(r'\[[^\]]*\]', '', declarator))[-1]
                       for declaration in body.split(';') if declaration.strip() for declarator in declaration.split(',')]
    return found


@functools.lru_cache(maxsize=None)
def make_database():
    """`make -pn` in csrc/: every variable and rule as make sees them; builds nothing."""
    return subprocess.run(['make', '-pn', '-C', CSRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          universal_newlines=True).stdout


def object_rule_prerequisites():
    rules = re.findall(r'^%\.o: %\.hip(.*)$', make_database(), flags=re.M)
    assert len(rules) == 1, rules
    return rules[0].split()


def host_cc():
    """$CC, else cc, else the clang that ships beside the Makefile's HIPCC.  build() cannot work without a compiler
    either, so finding none is a failure."""
    hipcc = re.search(r'^HIPCC\s*\??:?=\s*(\S+)', make_database(), flags=re.M)
    beside = os.path.join(os.path.dirname(os.path.realpath(hipcc.group(1))), '..', 'lib', 'llvm', 'bin', 'clang') if hipcc else ''
    for cc in (os.environ.get('CC'), 'cc', beside):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    raise AssertionError('no host C compiler: $CC, cc and %r are all missing' % beside)


def run_c99(lines, workdir):
    """Compiles `lines` as the body of main() of a C99 program that includes every header, runs it, and returns what it
    printed as {first word of a line: [the integers after it]}."""
    src = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in sorted(os.listdir(INCLUDE))]
    src += ['int main(void) {'] + list(lines) + ['return 0; }', '']
    c, exe = os.path.join(str(workdir), 'abi.c'), os.path.join(str(workdir), 'abi')
    open(c, 'w').write('\n'.join(src))
    subprocess.check_call([host_cc(), '-std=c99', '-I', INCLUDE, '-o', exe, c])
    out = subprocess.check_output([exe], universal_newlines=True)
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.splitlines()}
