// vh_params.hpp -- the ParameterFile reader of vh_params.cpp, for the other readers of zParameters*.txt files.
#pragma once

#include <istream>
#include <map>
#include <string>

namespace vh {

typedef std::map<std::string, std::string> ParamValues;

// addParameterFile (mLib parameterFile.h:22-60): "name = value" lines, comments and quotes removed; a later line
// overrides an earlier one
void parseStream(std::istream& in, ParamValues& values);

} // namespace vh
