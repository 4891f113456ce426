"""The reference's parser module (parser.py): ``Parser(name).get_tag(callback)`` / ``get_reader(callback)`` read one of its card files --
a JSON list of entries, `entry` tag / reader; for a tag `type` (ULTRALIGHT, else Classic 1K), `mem` and optional `rands`; for a reader
optional `rands`, `keya`, `keyb` -- into a tag.Tag / reader.Reader.  Without a file, or without the entry, the reference's defaults:
Tag.generate_1k's card, the FF keys."""
import json

from .command import TagType
from .reader import Reader
from .tag import Tag


class Parser(object):
    def __init__(self, name=None):
        if name:
            with open(name) as f:
                self._ar = json.load(f)
        else:
            self._ar = []

    def _entry(self, kind):
        return next((d for d in self._ar if d.get('entry', '') == kind), None)

    def get_reader(self, callback, **kw):   # (kw: Reader's keyword-only extras; positionally the reference's signature)
        d = self._entry('reader') or {}
        return Reader(callback, d.get('rands', []), d.get('keya', []), d.get('keyb', []), **kw)

    def get_tag(self, callback, **kw):      # (kw: Tag's keyword-only extras)
        d = self._entry('tag')
        if d is None:
            return Tag(callback, TagType.CLASSIC1K, Tag.generate_1k(), [], **kw)
        tag_type = TagType.ULTRALIGHT if d.get('type', '') == 'ULTRALIGHT' else TagType.CLASSIC1K
        return Tag(callback, tag_type, d.get('mem', []), d.get('rands', []), **kw)
