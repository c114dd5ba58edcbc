"""Extract the flag names / defaults / type names of the reference's train_vqvae.py as DATA (tests/golden/train_vqvae_cli_flags.json).

    python tests/golden/make_golden_vqvae_flags.py [path/to/reference/train_vqvae.py]

The argparse calls are read with ``ast`` (never imported or executed); only names, literal defaults and the type's name are kept
-- no source text.  Same kind of fixture as train_cli_flags.json (make_golden.py: cli_flags)."""

import ast
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent


def extract(ref: Path) -> dict:
    flags = {}
    for node in ast.walk(ast.parse(ref.read_text())):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            name = node.args[0].value.lstrip("-")
            kw = {k.arg: k.value for k in node.keywords}
            default = ast.literal_eval(kw["default"]) if "default" in kw else None
            typ = getattr(kw.get("type"), "id", None) or getattr(kw.get("type"), "attr", None)
            flags[name] = {"default": default, "type": typ}
    return flags


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    flags = extract(Path(sys.argv[1]))
    json.dump(flags, open(HERE / "train_vqvae_cli_flags.json", "w"), indent=1, sort_keys=True)
    print(f"{len(flags)} flags -> {HERE / 'train_vqvae_cli_flags.json'}")
