// kwage_amd/csrc/save_records.hpp -- the metadata records of the calls that write listed columns of a resident group to
// files (save.hip kwage_group_save_db: one `.db` file; export.hip kwage_group_export_bloom_files: a `.bloom` file per
// column): a kwage_save_column list turned into serialized FilterInfo records.  Host code only.
#ifndef KWAGE_AMD_SAVE_RECORDS_HPP
#define KWAGE_AMD_SAVE_RECORDS_HPP

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "host.hpp"
#include "internal.h"

namespace kwage {

// host.cpp
int sample_info_to_filter_info(const kwage_sample_info *si, FilterInfo &fi);

// The FilterInfo record of every listed column, one after the other in list order: copied verbatim from its `.db` /
// `.dbz` file (each distinct file opened once), or serialized from a kwage_sample_info as kwage_make_bloom does.  `who`:
// the call the messages name.
inline int collect_records(const char *who, const kwage_save_column *cols, uint32_t n, std::vector<uint64_t> &rec_len, std::vector<unsigned char> &recs)
{
	std::map<std::string, std::unique_ptr<DbInfo>> sources;
	rec_len.assign(n, 0);
	recs.clear();
	for(uint32_t i = 0; i < n; ++i){
		const kwage_save_column &c = cols[i];
		if(c.source_db){
			std::unique_ptr<DbInfo> &d = sources[c.source_db];
			if(!d){
				d.reset(new DbInfo());
				std::string err;
				if(!d->open(c.source_db, err) || !d->load(err)){ return fail(KWAGE_ERR_IO, "%s: %s", who, err.c_str()); }
			}
			if(c.source_column >= d->header.num_filter){
				return fail(KWAGE_ERR_ARG, "%s: entry %u: %s has no column %u", who, i, c.source_db, c.source_column);
			}
			const uint64_t l = d->info_loc[c.source_column];
			if(l < d->tail_start || l >= d->tail_start + d->tail.size()){ return fail(KWAGE_ERR_FORMAT, "%s: %s: bad metadata index", who, c.source_db); }
			const unsigned char *p = d->tail.data() + (l - d->tail_start);
			FilterInfo fi;
			size_t used = 0;
			if(!parse_filter_info(p, d->tail.size() - (l - d->tail_start), fi, &used)){ return fail(KWAGE_ERR_FORMAT, "%s: %s: bad FilterInfo record", who, c.source_db); }
			recs.insert(recs.end(), p, p + used);
			rec_len[i] = used;
		}
		else{
			FilterInfo fi;
			int rc = sample_info_to_filter_info(c.info, fi);
			if(rc){ return rc; }
			const size_t before = recs.size();
			pack_filter_info(fi, recs);
			rec_len[i] = recs.size() - before;
		}
	}
	return KWAGE_OK;
}

}  // namespace kwage

#endif
