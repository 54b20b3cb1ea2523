"""The reference the positions tests compare against: the fold of the issue's contract in plain Python, and a dict that
stands in for the positions_latest collection under the reference's statements (heatmap_stream.py:217-228)."""
import numpy as np


def fold(state, rows):
    """state: {(provider, vehicleId): (ts_us, lat, lon)}; rows: a batch's latest rows in ascending row order, each
    (provider, vehicleId, ts_us, lat, lon).  Row i of key k replaces state[k] iff k is absent or ts_us > state[k].ts_us."""
    for p, v, ts, lat, lon in rows:
        cur = state.get((p, v))
        if cur is None or ts > cur[0]:
            state[(p, v)] = (ts, lat, lon)
    return state


def latest_rows(prov, veh, ts):
    """indices (ascending) of the rows whose ts equals the max ts of their (provider, vehicleId) in the batch"""
    best = {}
    for i, k in enumerate(zip(prov, veh)):
        if k not in best or ts[i] > best[k]:
            best[k] = ts[i]
    return [i for i, k in enumerate(zip(prov, veh)) if ts[i] == best[k]]


def apply_ops(coll, ops):
    """Apply UpdateOne ops (pymongo objects, or anything with _filter / _doc) to coll {_id: doc} in order, the way
    MongoDB does for these statements: the filter {_id, $or: [{ts: {$exists: false}}, {ts: {$lt: ts}}]} matches the
    document of that _id if it has no ts or an older one; a match is $set; no match upserts a document from the
    filter's equality fields plus $set -- which fails with a duplicate key when the _id exists (the filter matched
    nothing because ts was not older), and then changes nothing."""
    for op in ops:
        f, u = op._filter, op._doc["$set"]
        (no_ts, older) = f["$or"]
        assert no_ts == {"ts": {"$exists": False}}
        bound = older["ts"]["$lt"]
        doc = coll.get(f["_id"])
        if doc is None:
            coll[f["_id"]] = dict(_id=f["_id"], **u)
        elif "ts" not in doc or doc["ts"] < bound:
            doc.update(u)
    return coll


class Batch:
    """A micro-batch of (provider, vehicleId, ts_us, lat, lon) rows with dictionaries of its own: `p_order` / `v_order`
    fix the code order (default: first appearance), so that the same string gets another code in another batch."""

    def __init__(self, rows, p_order=None, v_order=None, extra_vehicles=()):
        self.rows = list(rows)
        self.prov = [r[0] for r in self.rows]
        self.veh = [r[1] for r in self.rows]
        self.ts = np.array([r[2] for r in self.rows], np.int64)
        self.lat = np.array([r[3] for r in self.rows], np.float64)
        self.lon = np.array([r[4] for r in self.rows], np.float64)
        self.providers = list(p_order) if p_order is not None else list(dict.fromkeys(self.prov))
        self.vehicles = (list(v_order) if v_order is not None else list(dict.fromkeys(self.veh))) + list(extra_vehicles)
        pi = {s: k for k, s in enumerate(self.providers)}
        vi = {s: k for k, s in enumerate(self.vehicles)}
        nv = max(len(self.vehicles), 1)
        self.vkey = np.array([pi[p] * nv + vi[v] for p, v in zip(self.prov, self.veh)], np.uint64)

    def latest(self):
        return [self.rows[i] for i in latest_rows(self.prov, self.veh, self.ts)]


def run(eng, epoch, b, update=True):
    """process the batch on the engine and fold its latest rows into the engine's positions state"""
    res = eng.process_batch(epoch, b.lat, b.lon, b.ts, vkey=b.vkey, row_valid=np.ones(len(b.rows), bool))
    assert res.latest_rows.tolist() == latest_rows(b.prov, b.veh, b.ts)
    if update:
        eng.update_positions(b.providers, b.vehicles)
    return res


def exported(eng):
    """the engine's positions state keyed by the string pair, lat / lon as their bit patterns"""
    recs, providers, vehicles = eng.positions()
    out = {}
    for r in recs:
        k = (providers[int(r["provider"])], vehicles[int(r["vehicle"])])
        assert k not in out, f"key {k} exported twice"
        out[k] = (int(r["ts_us"]), r["lat"].tobytes(), r["lon"].tobytes())
    return out


def bits(state):
    return {k: (int(ts), np.float64(lat).tobytes(), np.float64(lon).tobytes()) for k, (ts, lat, lon) in state.items()}
