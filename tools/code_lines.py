#!/usr/bin/env python3
"""Code lines of Python files: lines that carry at least one token other than a comment, outside module, class and function
docstrings.  ``python tools/code_lines.py FILE...`` prints one count per file and the total; with ``--rev REV`` the files are read from
that git revision (a file that does not exist there counts 0), so that two commits can be put side by side."""
import argparse
import ast
import io
import subprocess
import sys
import tokenize

SKIP = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENCODING, tokenize.ENDMARKER)


def code_lines(source):
    """The number of code lines of a module's source text."""
    doc = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body:
            first = node.body[0]
            if isinstance(first, ast.Expr) and isinstance(first.value, ast.Constant) and isinstance(first.value.value, str):
                doc.update(range(first.lineno, first.end_lineno + 1))
    lines = set()
    for tok in tokenize.generate_tokens(io.StringIO(source).readline):
        if tok.type not in SKIP:
            lines.update(range(tok.start[0], tok.end[0] + 1))
    return len(lines - doc)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('files', nargs='+')
    ap.add_argument('--rev', help='read the files from this git revision instead of the working tree')
    args = ap.parse_args()
    total = 0
    for path in args.files:
        if args.rev:
            got = subprocess.run(['git', 'show', '%s:%s' % (args.rev, path)], capture_output=True, text=True)
            source = got.stdout if got.returncode == 0 else ''
        else:
            with open(path) as f:
                source = f.read()
        n = code_lines(source)
        total += n
        print('%6d  %s' % (n, path))
    print('%6d  total' % total)


if __name__ == '__main__':
    sys.exit(main())
