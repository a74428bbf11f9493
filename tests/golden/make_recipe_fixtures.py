"""Store the reference's recipe DATA files as one JSON fixture, so that tests/test_recipes.py and tests/test_text.py run
from a checkout of this repository alone (run in the build container only; the GPU box has no /root/reference).

Stored (data, not code):
  arch  every recipes/**/*.arch file, text as is, keyed by its path under recipes/
  cfg   every recipes/**/*.cfg file (gflags flags files), same keying
  conv_glu_prepare   what recipes/conv_glu/librispeech/prepare.py:59-84 WRITES: the lines of tokens.txt and one
                     lexicon line in its format -- the script's fixed output, checked here against the script before it
                     is stored.
    python tests/golden/make_recipe_fixtures.py
"""
import glob
import json
import os

REF = "/root/reference/recipes"
OUT = os.path.dirname(os.path.abspath(__file__))


def _files(pattern):
    return {os.path.relpath(f, REF): open(f).read() for f in sorted(glob.glob(f"{REF}/**/{pattern}", recursive=True))}


def main():
    src = open(os.path.join(REF, "conv_glu", "librispeech", "prepare.py")).read()
    assert 'fout.write("|\\n")' in src and "fout.write(\"'\\n\")" in src and 'range(ord("a"), ord("z") + 1)' in src
    assert '"{word}\\t{tokens} |\\n"' in src
    word = "hello"
    prepare = dict(tokens=["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)],
                   lexicon_line="{word}\t{tokens} |\n".format(word=word, tokens=" ".join(list(word))),
                   source="recipes/conv_glu/librispeech/prepare.py:59-84")
    fixture = dict(arch=_files("*.arch"), cfg=_files("*.cfg"), conv_glu_prepare=prepare)
    assert len(fixture["arch"]) >= 30 and len(fixture["cfg"]) >= 100
    json.dump(fixture, open(os.path.join(OUT, "reference_recipes.json"), "w"), indent=0, sort_keys=True)
    print(len(fixture["arch"]), "arch files,", len(fixture["cfg"]), "cfg files")


if __name__ == "__main__":
    main()
