"""What include/istvt_hip.h declares, read from its text, for tests/test_abi_cpu.py: the prototypes as ctypes argument lists,
the structs field by field, the integer #defines, and the comparisons against the hand-written table of istvt_amd._lib.
Everything takes the header TEXT, so a test can feed a doctored copy and watch the comparison fail."""
import ctypes
import re

# the one table from a spelled C type to ctypes; any pointer is c_void_p except a pointer to an argument block
SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double,
           'unsigned long long': ctypes.c_ulonglong, 'istvt_stream_t': ctypes.c_void_p}


class AbiError(AssertionError):
    pass


def strip_comments(text):
    return re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))


def _spelling(words):
    """'const  void * const *' -> 'const void*const*'"""
    return re.sub(r'\s*\*\s*', '*', ' '.join(words.split()))


def _declarator(decl, where):
    """'const void* const* dy' -> ('const void*const*', 'dy', None);  'int reserved[3]' -> ('int', 'reserved', 3)"""
    m = re.fullmatch(r'(.*[\s*])(\w+)\s*(?:\[(\d+)\])?', decl.strip(), re.S)
    if not m or not m.group(1).strip():
        raise AbiError('%s: cannot read the declaration %r' % (where, decl.strip()))
    return _spelling(m.group(1)), m.group(2), int(m.group(3)) if m.group(3) else None


def ctype_of(spelling, blocks, where):
    """blocks: {struct name: its ctypes.Structure}.  A spelling outside the table is an error, never a skip."""
    if spelling.endswith('*'):
        m = re.fullmatch(r'const (\w+)\*', spelling)
        return ctypes.POINTER(blocks[m.group(1)]) if m and m.group(1) in blocks else ctypes.c_void_p
    if spelling not in SCALARS:
        raise AbiError('%s: the type %r is not in the table' % (where, spelling))
    return SCALARS[spelling]


def prototypes(text):
    """{name: [(spelled type, parameter name)]} of every `int istvt_*(...);`"""
    out = {}
    for name, params in re.findall(r'\bint\s+(istvt_\w+)\s*\(([^()]*)\)\s*;', strip_comments(text)):
        if name in out:
            raise AbiError('%s is declared twice' % name)
        params = params.strip()
        out[name] = [] if params == 'void' else [_declarator(p, name)[:2] for p in params.split(',')]
    return out


def structs(text):
    """{name: [(spelled type, field name, array length or None)]} of every `typedef struct name {...} name;`"""
    out = {}
    for name, body in re.findall(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', strip_comments(text), re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            first, *more = decl.split(',')                      # `int n, nseg, nq`: one type, several names
            spelling, field, count = _declarator(first, name)
            fields.append((spelling, field, count))
            for extra in more:
                m = re.fullmatch(r'\s*(\w+)\s*(?:\[(\d+)\])?\s*', extra)
                if not m:
                    raise AbiError('%s: cannot read the field %r' % (name, extra))
                fields.append((spelling, m.group(1), int(m.group(2)) if m.group(2) else None))
        out[name] = fields
    return out


def defines(text):
    """{name: value} of the #defines whose value is one integer, bare or in parentheses"""
    found = re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', strip_comments(text), re.M)
    return {name: int(value) for name, value in found}


def signature_mismatches(text, table, blocks):
    """what separates the header's prototypes from `table` ({name: argtypes}), one line per entry point or argument"""
    bad, protos = [], prototypes(text)
    for name in sorted(set(protos) ^ set(table)):
        bad.append('%s: %s' % (name, 'declared, not in the table' if name in protos else 'in the table, not declared'))
    for name in sorted(set(protos) & set(table)):
        want = [ctype_of(t, blocks, '%s(%s)' % (name, p)) for t, p in protos[name]]
        if len(want) != len(table[name]):
            bad.append('%s: %d parameters declared, %d in the table' % (name, len(want), len(table[name])))
            continue
        for i, ((spelled, param), w, got) in enumerate(zip(protos[name], want, table[name])):
            if w is not got:
                bad.append('%s: argument %d (%s) is declared %s = %s, the table has %s'
                           % (name, i, param, spelled, w.__name__, got.__name__))
    return bad


def struct_mismatches(text, name, cls, blocks):
    """what separates the header's struct `name` from the ctypes.Structure `cls`: names, order and types"""
    declared = structs(text).get(name)
    if declared is None:
        return ['%s: not declared' % name]
    if any(count is not None for _, _, count in declared):
        return ['%s: array fields are not bound' % name]
    want = [(field, ctype_of(t, blocks, '%s.%s' % (name, field))) for t, field, _ in declared]
    got = [(f[0], f[1]) for f in cls._fields_]
    bad = []
    if len(want) != len(got):
        bad.append('%s: %d fields declared, %d in %s' % (name, len(want), len(got), cls.__name__))
    for i, (w, g) in enumerate(zip(want, got)):
        if w[0] != g[0] or w[1] is not g[1]:
            bad.append('%s: field %d is declared %s %s, %s has %s %s'
                       % (name, i, w[1].__name__, w[0], cls.__name__, g[1].__name__, g[0]))
    return bad


def layout_program(text, names):
    """a C program that prints `name sizeof` and `name.field offsetof` for the named structs of the header"""
    declared = structs(text)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "istvt_hip.h"', 'int main(void) {']
    for name in names:
        lines.append('    printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name))
        for _, field, _ in declared[name]:
            lines.append('    printf("%s.%s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (name, field, name, field))
    return '\n'.join(lines + ['    return 0;', '}', ''])
