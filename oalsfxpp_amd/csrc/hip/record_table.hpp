// The record table: the host's half of a per-voice record that lives on the device and is set from the host (samplers, voice
// envelopes, resamplers, voice filters, envelope programs: batch.cpp, DeviceRecords).  The table keeps what the host last knew of
// every row and which rows it has set since they last went to the device:
//
//     set(i, value)            the host's row is the current one from here on; the row is marked and listed once, however often it is set
//     drain(changed, index)    the listed rows and their instance numbers, in list order, into the two arrays of a staging buffer that
//                              one launch scatters to the device; marks and list are cleared
//     merge(device_rows)       a read-back: the device's value for every row that is not marked
//
// What a row means (which rows count as active, which values are refused) is the caller's business.  Plain C++, no HIP types:
// tests/test_record_table.py drives the table against a plain array that stands for the device.
#ifndef OALSFX_RECORD_TABLE_HPP
#define OALSFX_RECORD_TABLE_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace oalsfx_records {

template <class T>
class RecordTable {
public:
    std::vector<T> host; // [n] as set, or as last read back

    void assign(size_t n, const T& init)
    {
        host.assign(n, init);
        dirty.assign(n, 0);
        dirty_list.clear();
    }

    void set(int i, const T& value)
    {
        host[i] = value;
        if (!dirty[i]) {
            dirty[i] = 1;
            dirty_list.push_back(i);
        }
    }

    // Whether row i was set since the last drain: the host's row is the current one.
    bool is_set(int i) const { return dirty[i] != 0; }

    // Rows set since the last drain.
    size_t pending() const { return dirty_list.size(); }

    // How many records the staging buffer of the next drain holds: the `capacity` there is, or, where that is too small for the pending
    // rows, twice their number and 64 at least -- a caller that sets a few more rows every time does not allocate every time -- but
    // never more than the table has rows.
    size_t staging_capacity(size_t capacity) const
    {
        const size_t count = pending();
        return count <= capacity ? capacity : std::min<size_t>(host.size(), std::max<size_t>(2 * count, 64));
    }

    // changed[k], index[k], k < pending(): room for staging_capacity() entries each.
    void drain(T* changed, int* index)
    {
        for (size_t k = 0; k < dirty_list.size(); ++k) {
            const int i = dirty_list[k];
            index[k] = i;
            changed[k] = host[i];
            dirty[i] = 0;
        }
        dirty_list.clear();
    }

    // device_rows, [n], as the device holds them behind everything drained so far: what was set since then is the host's.
    void merge(const T* device_rows)
    {
        for (size_t i = 0; i < host.size(); ++i)
            if (!dirty[i]) host[i] = device_rows[i];
    }

private:
    std::vector<uint8_t> dirty;  // [n] set since the last drain: the host's row is the current one
    std::vector<int> dirty_list; // ... which, in the order they were first set
};

} // namespace oalsfx_records

#endif // OALSFX_RECORD_TABLE_HPP
