"""What the ABI ledgers of the test_*_cpu.py files share: the headers under include/ as name -> argument count, Python source
reduced to its code, the walk over every `lib.X('mmft_...', ...)` call site, and the table of the extension headers.  A plain
module: it holds no test."""
import ast
import glob
import io
import os
import re
import tokenize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'multimodal-fusion-based-pre-routing-timing-prediction-_amd')

# accessor of mmft.lib -> the extension header it binds.  One row per lib.Header instance; test_abi_ledger_cpu.py holds the
# two against each other.
HEADERS = {'ext': 'mmft_report.h', 'place': 'mmft_place.h', 'incr': 'mmft_incr.h', 'crit': 'mmft_crit.h', 'head': 'mmft_head.h',
           'csum': 'mmft_crit_sums.h', 'sens': 'mmft_sens.h', 'simg': 'mmft_sens_image.h', 'pmove': 'mmft_sens_pins.h'}


def others(header):
    """Every header a new name in `header` could collide with: the other extension headers and mmft.h."""
    return ['mmft.h'] + [h for h in HEADERS.values() if h != header]


def declared(header):
    """{name: number of parameters} of every function a header under include/ declares (comments stripped)."""
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r'\b(?:int|long long|const char\*)\s+(mmft_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', hdr, re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ('', 'void') else len(args.split(','))
    return protos


def code_only(src):
    """Python source without comments and docstrings: what is left are names and the string literals that code uses."""
    doc = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.FunctionDef, ast.ClassDef)) and node.body and isinstance(node.body[0], ast.Expr) and \
                isinstance(node.body[0].value, ast.Constant) and isinstance(node.body[0].value.value, str):
            doc.add(node.body[0].lineno)
    out = []
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type == tokenize.COMMENT or (tok.type == tokenize.STRING and tok.start[0] in doc):
            continue
        out.append(tok.string)
    return ' '.join(out)


def call_sites(attrs, bench=False):
    """(name, nargs, file, lineno) of every `something.<attr>('mmft_...', ...)` call, attr in `attrs`, in the package, tests/*.py,
    tools/*.py and, with `bench`, bench.py.  nargs counts the arguments after the name, a starred `stream_args(...)` as its
    two (device, stream); it is None where another starred argument - a list built elsewhere - makes the count unknowable."""
    attrs = (attrs,) if isinstance(attrs, str) else tuple(attrs)
    files = glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True)
    files += glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py'))
    files += [os.path.join(ROOT, 'bench.py')] if bench else []
    for f in files:
        for node in ast.walk(ast.parse(open(f).read())):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in attrs and node.args
                    and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str) and node.args[0].value.startswith('mmft_')):
                continue
            n = 0
            for a in node.args[1:]:
                if not isinstance(a, ast.Starred):
                    n += 1
                elif isinstance(a.value, ast.Call) and getattr(a.value.func, 'attr', '') == 'stream_args':
                    n += 2
                else:
                    n = None
                    break
            yield node.args[0].value, n, f, node.lineno
